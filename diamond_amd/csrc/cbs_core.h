// cbs_core.h -- composition-based matrix adjustment of one (query, target) pair as ONE WAVEFRONT computes it: the code of
// cbs_adjust_kernel (cbs_kernels.hip) and, run lane after lane on the CPU, of the lane emulator (tests/emu/cbs_emu.cpp).
//
// The arithmetic is cbs_adjust.cpp's (the host form, which stays the second implementation): the target's composition, the
// rule of cbs_rule and, for CBS_RULE_REL_ENTROPY, the table of cbs_target_matrix. How it is laid out over 64 lanes:
//   * the 400-vectors (x, the gradients, the residuals, D^-1) are strided over the lanes, element k on lane k % 64;
//   * everything that another lane reads lives in the wavefront's workspace (CbsWave, in LDS on the device), and the code is
//     a sequence of phases -- CBS_LANES(l) { what lane l does } CBS_SYNC() -- in which no lane reads what another lane writes
//     in the same phase. So the emulator may run the lanes of a phase one after the other and gets the device's doubles;
//   * whatever a lane reads outside CBS_LANES comes from the workspace or from arguments alike for all lanes, so those
//     scalars hold one value for the whole wavefront and every branch on them is taken by all 64 lanes;
//   * the 39 marginal sums (A x, A D^-1 A^T) are 20 additions each, one lane per sum, in the host's order; the Cholesky
//     factorisation goes column by column, lane i holding row i and subtracting the products of the earlier columns in the
//     host's order; both triangular solves go column by column as well. Given the same inputs these give the host's doubles;
//   * the sums over all 400 elements (the relative entropy, the squared residual norm, grad^T D^-1 grad, the sum of the
//     target frequencies) are a partial sum per lane and a binary tree over the 64 partial sums. These do NOT add in the
//     host's order, and the device's log / acos are not glibc's, so a double may differ from the host's in its last bits.
// The rounded table must be the reference's all the same. Hence the guards: wherever a decision (a rounding to an integer, the
// convergence test, the rule's angle test) lies so close to its threshold that such last-bit differences could flip it, the
// pair gets a non-zero status, nothing is written, and the host computes it (extend_host.hip). Widths: DESIGN.md 4.13,
// profiles/cbs_device_guards.json.
//
// Decisions that need no guard, because both sides evaluate them on identical doubles:
//   * the composition: exact integer counts, one correctly rounded division count / n each (cbs_composition does the same);
//   * high_pair: those quotients, compared with each other (exact) and one correctly rounded sum of two of them against 0.4;
//   * the length ratio: two exact integers, one correctly rounded division, against a constant;
//   * the pseudocount mix: 20 additions in the host's order on the host's inputs.
// Keep the operation order of these few expressions as cbs_adjust.cpp has it. Compile with -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <limits.h>
#include <math.h>

#if defined(__HIPCC__)
#define CBS_FN __host__ __device__ inline
#else
#define CBS_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define CBS_LANES(l) if (const int l = (int)(threadIdx.x & 63); true)
#define CBS_SYNC() __syncthreads()
#define CBS_COUNT(p) atomicAdd((p), 1)
#else
#define CBS_LANES(l) for (int l = 0; l < 64; ++l)
#define CBS_SYNC() ((void)0)
#define CBS_COUNT(p) (++*(p))
#endif

namespace dmnd {

enum { CBSD_N = 20, CBSD_NN = 400, CBSD_M = 40, CBSD_X = 23, CBSD_S = 21, CBSD_LTRI = CBSD_M * (CBSD_M + 1) / 2 };
enum { CBSD_RULE_NONE = -1, CBSD_RULE_SCALE_OLD = 0, CBSD_RULE_REL_ENTROPY = 4 };      // = CBS_RULE_* of cbs_adjust.h
// who computes the pair: 0 = the device did; otherwise the guard that handed it back to the host
enum { CBS_ST_DEVICE = 0, CBS_ST_ROUNDING = 1, CBS_ST_ITERATIONS = 2, CBS_ST_RULE = 3 };

// Guard widths and the device's iteration cap, from the measurement of profiles/cbs_device_guards.json: each
// width is at least 1000 x the largest deviation between this schedule (lane emulator) and the host arithmetic.
#define CBS_EPS_ROUND 1e-7          // absolute, in score units: distance of an unrounded score from a .5 boundary
#define CBS_EPS_NORM  1e-3          // relative to err_tolerance: band around the convergence threshold (and around z[39] < 1)
#define CBS_EPS_ANGLE 1e-7          // degrees: band around the angle threshold of the conditioned modes
#define CBS_EPS_ARG   1e-9          // the acos argument of that angle: closer to -1 than this, acos is 180 degrees on one side and may be NaN on the other
#define CBS_DEVICE_MAX_ITS 64       // Newton steps a wavefront spends on one pair before it hands it back

// what the kernel reads of a CbsModel, plus the guards
struct CbsDevModel {
	double joint_probs[CBSD_NN], background[CBSD_N];
	double lambda;                    // ideal_lambda / scale
	double err_tolerance, angle, distance_threshold, length_ratio_threshold;
	double eps_round, eps_norm, eps_angle;
	int32_t mode, scale, max_its, pad;
	int8_t matrix8[32 * 32];
};

// workspace of one wavefront: 25.4 KB (six wavefronts per CU in 160 KB of LDS)
struct CbsWave {
	double x[CBSD_NN], old_scores[CBSD_NN], grad1[CBSD_NN], rx[CBSD_NN], Dinv[CBSD_NN];
	double L[CBSD_LTRI];              // lower triangle, row i at i (i + 1) / 2
	double z[CBSD_M], rz[CBSD_M], zs[CBSD_M], tmp[CBSD_M];
	double row[CBSD_N], col[CBSD_N], tc[CBSD_N], sxr[CBSD_N], sxc[CBSD_N], avg[CBSD_N];
	double red[64], red2[64];
	int cnt[CBSD_N];
	int flag;
};

// what the emulator exports beside the results (never set on the device)
struct CbsEmuTrace {
	enum { CAP = 256 };
	double rnorm[CAP];
	int n_rnorm, its;
	double angle;
};

CBS_FN double& cbsd_L(CbsWave& W, int i, int j) { return W.L[i * (i + 1) / 2 + j]; }

// tree over red[0 .. 64): the device's order of addition
CBS_FN double cbsd_reduce_sum(double* red)
{
	for (int s = 32; s > 0; s >>= 1) {
		CBS_LANES(l) { if (l < s) red[l] += red[l + s]; }
		CBS_SYNC();
	}
	const double r = red[0];
	CBS_SYNC();
	return r;
}

CBS_FN double cbsd_reduce_min(double* red)
{
	for (int s = 32; s > 0; s >>= 1) {
		CBS_LANES(l) { if (l < s && red[l + s] < red[l]) red[l] = red[l + s]; }
		CBS_SYNC();
	}
	const double r = red[0];
	CBS_SYNC();
	return r;
}

// composition_distance of cbs_adjust.cpp, one lane
CBS_FN double cbsd_distance(const double* A, const double* B)
{
	double value = 0.0;
	for (int i = 0; i < CBSD_N; ++i) {
		const double t = (A[i] + B[i]) / 2;
		if (t > 0) {
			if (A[i] > 0) value += A[i] * log(A[i] / t) / 2;
			if (B[i] > 0) value += B[i] * log(B[i] / t) / 2;
		}
	}
	if (value < 0) value = 0;
	return sqrt(value);
}

// high_pair of cbs_adjust.cpp (no guard: see the head of the file)
CBS_FN bool cbsd_high_pair(const double* p, int length)
{
	if (length <= 50) return false;
	double max = 0, second = 0;
	for (int i = 0; i < CBSD_N; ++i)
		if (p[i] > second) {
			second = p[i];
			if (p[i] > max) { second = max; max = p[i]; }
		}
	return (max + second) > 0.4;
}

// apply_pseudocounts of cbs_adjust.cpp, one lane
CBS_FN void cbsd_pseudocounts(double* out, const double* probs, int observations, const double* background)
{
	double sum = 0.0;
	for (int i = 0; i < CBSD_N; ++i) sum += probs[i];
	if (sum == 0.0) sum = 1.0;
	const double weight = 20.0 / (observations + 20.0);
	for (int i = 0; i < CBSD_N; ++i)
		out[i] = (1.0 - weight) * probs[i] / sum + weight * background[i];
}

CBS_FN int cbsd_round_score(double f) { return f < INT_MIN ? INT_MIN : (int)round(f); }

// The Newton system of one iteration: D^-1, J D^-1 J^T and its Cholesky factor (kkt_factor of cbs_adjust.cpp)
CBS_FN void cbsd_factor(CbsWave& W, double eta)
{
	const int N = CBSD_N;
	const double om = 1 - eta;
	CBS_LANES(l) {
		double p = 0.0;
		for (int k = l; k < CBSD_NN; k += 64) {
			const double d = W.x[k] / om;
			W.Dinv[k] = d;
			p += W.grad1[k] * (d * W.grad1[k]);
		}
		W.red[l] = p;
		for (int e = l; e < CBSD_LTRI; e += 64) W.L[e] = 0.0;
	}
	CBS_SYNC();
	const double gdg = cbsd_reduce_sum(W.red);
	CBS_LANES(l) {
		if (l < N) {                                      // column sum j = l of D^-1 and of D^-1 grad
			double d = 0.0, w = 0.0;
			for (int i = 0; i < N; ++i) { const double dd = W.Dinv[i * N + l]; d += dd; w += 1.0 * (dd * W.grad1[i * N + l]); }
			cbsd_L(W, l, l) = d;
			cbsd_L(W, CBSD_M - 1, l) = w;
		}
		else if (l < CBSD_M - 1) {                        // row sum i = l - 19, and the row's entries below the first block
			const int i = l - (N - 1);
			double d = 0.0, w = 0.0;
			for (int j = 0; j < N; ++j) { const double dd = W.Dinv[i * N + j]; cbsd_L(W, l, j) = dd; d += dd; w += 1.0 * (dd * W.grad1[i * N + j]); }
			cbsd_L(W, l, l) = d;
			cbsd_L(W, CBSD_M - 1, l) = w;
		}
		else if (l == CBSD_M - 1) cbsd_L(W, l, l) = gdg;
	}
	CBS_SYNC();
	for (int j = 0; j < CBSD_M; ++j) {
		CBS_LANES(l) {
			if (l >= j && l < CBSD_M) {
				double t = cbsd_L(W, l, j);
				for (int k = 0; k < j; ++k) t -= cbsd_L(W, l, k) * cbsd_L(W, j, k);
				W.tmp[l] = t;
			}
		}
		CBS_SYNC();
		CBS_LANES(l) {
			if (l >= j && l < CBSD_M) {
				const double d = sqrt(W.tmp[j]);
				cbsd_L(W, l, j) = l == j ? d : W.tmp[l] / d;
			}
		}
		CBS_SYNC();
	}
}

// in: dual residuals rx, primal residuals rz; out: the Newton step in both (kkt_solve of cbs_adjust.cpp)
CBS_FN void cbsd_solve(CbsWave& W)
{
	const int N = CBSD_N;
	CBS_LANES(l) {
		double p = 0.0;
		for (int k = l; k < CBSD_NN; k += 64) p += W.grad1[k] * (W.rx[k] * W.Dinv[k]);
		W.red[l] = p;
		if (l < N) {
			double y = W.rz[l];
			for (int i = 0; i < N; ++i) y += -1.0 * (W.rx[i * N + l] * W.Dinv[i * N + l]);
			W.rz[l] = y;
		}
		else if (l < CBSD_M - 1) {
			const int i = l - (N - 1);
			double y = W.rz[l];
			for (int j = 0; j < N; ++j) y += -1.0 * (W.rx[i * N + j] * W.Dinv[i * N + j]);
			W.rz[l] = y;
		}
	}
	CBS_SYNC();
	const double gw = cbsd_reduce_sum(W.red);
	CBS_LANES(l) { if (l == CBSD_M - 1) W.rz[l] -= gw; }
	CBS_SYNC();
	for (int j = 0; j < CBSD_M; ++j) {                    // L y = b, a column at a time
		CBS_LANES(l) {
			if (l >= j && l < CBSD_M) {
				const double zj = W.rz[j] / cbsd_L(W, j, j);
				if (l == j) W.zs[j] = zj;
				else W.rz[l] -= cbsd_L(W, l, j) * zj;
			}
		}
		CBS_SYNC();
	}
	for (int j = CBSD_M - 1; j >= 0; --j) {               // L^T z = y
		CBS_LANES(l) {
			if (l <= j) {
				const double zj = W.zs[j] / cbsd_L(W, j, j);
				if (l == j) W.rz[j] = zj;
				else W.zs[l] -= cbsd_L(W, j, l) * zj;
			}
		}
		CBS_SYNC();
	}
}

// One pair. target: tlen letters; table_out: the pair's 32 x 32 slot, written only with status 0 and rule REL_ENTROPY;
// scores_out (optional): the 21 x 21 unrounded scores [query letter][target letter], index 20 = the mask letter, written
// whenever the optimisation converged; rule_out / status_out: always written.
CBS_FN void cbsd_pair(CbsWave& W, const CbsDevModel& m, const double* qcomp, int q_true_aa, const int8_t* target, int tlen,
	int8_t* table_out, double* scores_out, int32_t* rule_out, uint8_t* status_out, CbsEmuTrace* tr)
{
	const int N = CBSD_N;
	const double* q = m.joint_probs;
	int rule = CBSD_RULE_NONE, status = CBS_ST_DEVICE;
	const bool adjust = m.mode >= 2 && m.mode <= 6, conditioned = m.mode == 2 || m.mode == 3 || m.mode == 5 || m.mode == 6;
	if (tr) { tr->n_rnorm = 0; tr->its = 0; tr->angle = 0.0; }
	if (adjust && tlen > 0 && q_true_aa != 0) {
		// ---- the target's composition ----
		CBS_LANES(l) { if (l < N) W.cnt[l] = 0; if (l == 0) W.flag = 0; }
		CBS_SYNC();
		CBS_LANES(l) {
			for (int p = l; p < tlen; p += 64) { const int a = target[p] & 31; if (a < N) CBS_COUNT(&W.cnt[a]); }
		}
		CBS_SYNC();
		int n = 0;
		for (int i = 0; i < N; ++i) n += W.cnt[i];
		CBS_LANES(l) { if (l < N) W.tc[l] = n == 0 ? 0.0 : (double)W.cnt[l] / n; }
		CBS_SYNC();
		// ---- the rule (cbs_rule) ----
		rule = CBSD_RULE_REL_ENTROPY;
		if (conditioned) {
			CBS_LANES(l) {
				if (l == 0) W.red[0] = cbsd_distance(W.tc, m.background);
				else if (l == 1) W.red[1] = cbsd_distance(qcomp, m.background);
				else if (l == 2) W.red[2] = cbsd_distance(W.tc, qcomp);
			}
			CBS_SYNC();
			const double d_m_mat = W.red[0], d_q_mat = W.red[1], d_m_q = W.red[2];
			CBS_SYNC();
			const double arg = (d_m_mat * d_m_mat + d_q_mat * d_q_mat - d_m_q * d_m_q) / 2.0 / d_m_mat / d_q_mat;
			double angle = acos(arg);
			angle = angle * 180 / 3.1415926543;
			if (tr) tr->angle = angle;
			const double len_q = 1.0 * q_true_aa, len_m = 1.0 * tlen;
			const double len_large = len_q > len_m ? len_q : len_m, len_small = len_q > len_m ? len_m : len_q;
			if (cbsd_high_pair(qcomp, q_true_aa) || cbsd_high_pair(W.tc, tlen)) rule = CBSD_RULE_REL_ENTROPY;
			else if (d_m_q > m.distance_threshold && len_large / len_small > m.length_ratio_threshold) {
				// the angle test is the one comparison here on doubles that went through log and acos. NaN (the quotient beyond
				// +-1 by a last bit, or a zero distance) compares false on both sides only where the quotient is at the +1 end. At the
				// -1 end one side may see 180 degrees and the other NaN, whichever of the two is a last bit beyond: a quotient within
				// CBS_EPS_ARG of -1 (or NaN itself) goes back, whatever its angle.
				if (!(arg > -1.0 + CBS_EPS_ARG) || (angle != angle ? !(arg >= 1.0) : !(fabs(angle - m.angle) > m.eps_angle))) status = CBS_ST_RULE;
				rule = angle > m.angle ? CBSD_RULE_SCALE_OLD : CBSD_RULE_REL_ENTROPY;
			}
			// (the two thresholds in front of the angle are -1 against values >= 0: no guard)
			if (m.mode != 5 && rule == CBSD_RULE_SCALE_OLD) rule = CBSD_RULE_NONE;
			if (rule == CBSD_RULE_SCALE_OLD) status = CBS_ST_RULE;      // lambda_rescale stays on the host
		}
		if (status == CBS_ST_DEVICE && rule == CBSD_RULE_REL_ENTROPY) {
			// ---- relative_entropy_adjust: pseudocounts, then optimise_target_freqs ----
			CBS_LANES(l) {
				if (l == 0) cbsd_pseudocounts(W.row, qcomp, q_true_aa, m.background);
				else if (l == 1) cbsd_pseudocounts(W.col, W.tc, n, m.background);
				else if (l >= 2 && l < 2 + CBSD_M) W.z[l - 2] = 0.0;
			}
			CBS_SYNC();
			CBS_LANES(l) {
				for (int k = l; k < CBSD_NN; k += 64) {
					W.old_scores[k] = log(q[k] / (W.row[k / N] * W.col[k % N]));
					W.x[k] = q[k];
				}
			}
			CBS_SYNC();
			const double re = 0.44, tol = m.err_tolerance;
			int its = 0;
			bool converged = false;
			for (;;) {
				const double eta = W.z[CBSD_M - 1];
				CBS_LANES(l) {
					double pv = 0.0, ps = 0.0;
					for (int k = l; k < CBSD_NN; k += 64) {
						const int i = k / N, j = k % N;
						double t = log(W.x[k] / q[k]);
						const double g0 = t + 1;
						t += W.old_scores[k];
						pv += W.x[k] * t;
						const double g1 = t + 1;
						W.grad1[k] = g1;
						double r = -g0 + eta * g1;
						r += 1.0 * W.z[j];
						if (i > 0) r += 1.0 * W.z[i + N - 1];
						W.rx[k] = r;
						ps += r * r;
					}
					W.red[l] = pv;
					W.red2[l] = ps;
				}
				CBS_SYNC();
				const double v1 = cbsd_reduce_sum(W.red);
				const double sx = cbsd_reduce_sum(W.red2);
				CBS_LANES(l) {
					if (l < N) {
						double y = W.col[l];
						for (int i = 0; i < N; ++i) y += -1.0 * W.x[i * N + l];
						W.rz[l] = y;
					}
					else if (l < CBSD_M - 1) {
						const int i = l - (N - 1);
						double y = W.row[i];
						for (int j = 0; j < N; ++j) y += -1.0 * W.x[i * N + j];
						W.rz[l] = y;
					}
					else if (l == CBSD_M - 1) W.rz[l] = re - v1;
				}
				CBS_SYNC();
				CBS_LANES(l) { W.red[l] = l < CBSD_M ? W.rz[l] * W.rz[l] : 0.0; }
				CBS_SYNC();
				const double sz = cbsd_reduce_sum(W.red);
				const double rnorm = sqrt(sx + sz);
				if (tr) { if (tr->n_rnorm < CbsEmuTrace::CAP) tr->rnorm[tr->n_rnorm++] = rnorm; tr->its = its; }
				if (!(fabs(rnorm - tol) > m.eps_norm * tol)) { status = CBS_ST_ITERATIONS; break; }      // in the band, or NaN
				if (!(rnorm > tol)) { converged = true; break; }
				if (++its > m.max_its) { status = CBS_ST_ITERATIONS; break; }
				cbsd_factor(W, eta);
				cbsd_solve(W);
				CBS_LANES(l) {
					double a = 1.0 / .95;
					for (int k = l; k < CBSD_NN; k += 64) {
						const int i = k / N, j = k % N;
						double r = W.rx[k];
						r += W.grad1[k] * W.rz[CBSD_M - 1];
						r += 1.0 * W.rz[j];
						if (i > 0) r += 1.0 * W.rz[i + N - 1];
						r *= W.Dinv[k];
						W.rx[k] = r;
						const double s = -W.x[k] / r;
						if (s >= 0 && s < a) a = s;
					}
					W.red[l] = a;
				}
				CBS_SYNC();
				double alpha = cbsd_reduce_min(W.red);
				alpha *= 0.95;
				CBS_LANES(l) {
					for (int k = l; k < CBSD_NN; k += 64) W.x[k] += alpha * W.rx[k];
					if (l < CBSD_M) W.z[l] += alpha * W.rz[l];
				}
				CBS_SYNC();
			}
			if (converged && !(W.z[CBSD_M - 1] < 1 - m.eps_norm)) { status = CBS_ST_ITERATIONS; converged = false; }
			if (converged) {
				// ---- scores_from_freqs ----
				CBS_LANES(l) {
					double p = 0.0;
					for (int k = l; k < CBSD_NN; k += 64) p += W.x[k];
					W.red[l] = p;
				}
				CBS_SYNC();
				const double sum = cbsd_reduce_sum(W.red);
				CBS_LANES(l) {
					for (int k = l; k < CBSD_NN; k += 64) {
						const int i = k / N, j = k % N;
						double s = W.x[k] / sum;
						if (W.row[i] > 0 && W.col[j] > 0) s /= (W.row[i] * W.col[j]);
						W.rx[k] = 0.0 == s ? -128.0 : log(s) / m.lambda;
					}
				}
				CBS_SYNC();
				CBS_LANES(l) {                                // set_x_scores
					if (l < N) {
						double avg = 0.0, c = 0.0;
						for (int j = 0; j < N; ++j) avg += W.rx[l * N + j] * W.col[j];
						for (int j = 0; j < N; ++j) c += W.rx[j * N + l] * W.row[j];
						W.avg[l] = avg;
						W.sxr[l] = avg < -1.0 ? avg : -1.0;
						W.sxc[l] = c < -1.0 ? c : -1.0;
					}
				}
				CBS_SYNC();
				double sxx = 0.0;
				for (int i = 0; i < N; ++i) sxx += W.avg[i] * W.row[i];
				sxx = sxx < -1.0 ? sxx : -1.0;
				// the rounding guard over all 21 x 21 scores (the mask letter's are -1 or an average below it: either way the
				// value that is rounded is the value tested here)
				CBS_LANES(l) {
					bool near = false;
					for (int e = l; e < CBSD_S * CBSD_S; e += 64) {
						const int a = e / CBSD_S, b = e % CBSD_S;
						const double v = a < N ? (b < N ? W.rx[a * N + b] : W.sxr[a]) : (b < N ? W.sxc[b] : sxx);
						if (scores_out) scores_out[e] = v;
						const double f = v - floor(v);
						if (!(fabs(f - 0.5) > m.eps_round)) near = true;
					}
					if (near) W.flag = 1;
				}
				CBS_SYNC();
				if (W.flag) status = CBS_ST_ROUNDING;
				else {
					// TargetMatrix::TargetMatrix as cbs_target_matrix stores it: out[target letter * 32 + query letter]
					CBS_LANES(l) {
						for (int e = l; e < 32 * 32; e += 64) {
							const int i = e >> 5, j = e & 31;
							int8_t v = -128;
							if (i < 26 && j < 26) {
								if ((i < N || i == CBSD_X) && (j < N || j == CBSD_X)) {
									const double s = j < N ? (i < N ? W.rx[j * N + i] : W.sxr[j]) : (i < N ? W.sxc[i] : sxx);
									v = (int8_t)cbsd_round_score(s);
								}
								else { const int s = m.matrix8[e] * m.scale; v = (int8_t)(s > SCHAR_MIN ? s : SCHAR_MIN); }
							}
							table_out[e] = v;
						}
					}
				}
				CBS_SYNC();
			}
		}
	}
	CBS_LANES(l) { if (l == 0) { *rule_out = rule; *status_out = (uint8_t)status; } }
	CBS_SYNC();
}

// ---- host-side slot bookkeeping of a dmnd_extend planning step (extend_host.hip; tests/asan/cbs_slots_main.cpp) --------------
// The step's new pairs take the slots [before, before + n) of the work context's matrix store in list order. After the kernel,
// rule[k] / status[k] say what became of pair k: its matrix number is -1 (the target keeps the standard matrix; the slot stays
// unused) or before + k, and the pairs whose status is not 0 are listed for the host threads, which write their tables into
// patch[(position in the list) * 1024] for one copy per run of consecutive slots.
struct CbsPatchRun { int64_t first_slot, first_patch, n; };

// fills mat_of[k] and the hand-back list; returns the number of handed-back pairs that need a table. by_status[4]: pairs per status.
inline int64_t cbs_slots_assign(int64_t before, int64_t n, const int32_t* rule, const uint8_t* status, int32_t* mat_of, int64_t* handed, int64_t* by_status)
{
	int64_t h = 0;
	for (int k = 0; k < 4; ++k) by_status[k] = 0;
	for (int64_t k = 0; k < n; ++k) {
		const int st = status[k] < 4 ? status[k] : CBS_ST_ITERATIONS;
		++by_status[st];
		if (st != CBS_ST_DEVICE) { handed[h++] = k; mat_of[k] = (int32_t)(before + k); }      // the host decides the rule as well: may still become -1
		else mat_of[k] = rule[k] == CBSD_RULE_NONE ? -1 : (int32_t)(before + k);
	}
	return h;
}

// runs of consecutive slots among handed[0 .. h) whose host rule is not NONE (keep[i] != 0): one copy each. runs has room for h.
inline int64_t cbs_patch_runs(int64_t before, const int64_t* handed, const uint8_t* keep, int64_t h, CbsPatchRun* runs)
{
	int64_t r = 0;
	for (int64_t i = 0; i < h; ++i) {
		if (!keep[i]) continue;
		if (r > 0 && runs[r - 1].first_slot + runs[r - 1].n == before + handed[i] && runs[r - 1].first_patch + runs[r - 1].n == i) ++runs[r - 1].n;
		else runs[r++] = CbsPatchRun{ before + handed[i], i, 1 };
	}
	return r;
}

}  // namespace dmnd
