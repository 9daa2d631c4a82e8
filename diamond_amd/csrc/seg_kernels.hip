// seg_kernels.hip -- SEG low-complexity masking of a block in HBM (`--masking seg`; host statement: seg_mask.h, arithmetic: seg_core.h).
//
//   seg_class_kernel      one wavefront per sequence, a lane per letter, 64 letters a step: the class (none / trigger / extend / break)
//                         of the 10-letter window centred at each letter into a byte of scratch; the sequences that hold a trigger
//                         window -- one in seven of real proteins -- are appended to the work list.
//   seg_segments_kernel   one wavefront per listed sequence runs seg_drive (seg::seg_seq) wave-uniformly: triggers and the ends of a
//                         raw segment are found by ballots over 64 classes at a time; the trim step's up to 1275 candidates go over
//                         the lanes, 64 a round, each from the raw segment's composition and the prefix / suffix compositions of its
//                         ends in LDS, and a butterfly keeps the smallest (value, order). Ranges are appended to a list whose counter
//                         keeps counting when the list is full; no letter is written here, because neighbouring segments overlap
//                         and every trim reads the original letters.
//   seg_apply_kernel      one wavefront per range writes the mask letter, once the host knows that the list is complete.
#pragma clang fp contract(off)
#include "seg_kernels.h"

namespace dmnd {

namespace {

__global__ __launch_bounds__(256) void seg_class_kernel(const SegArgs a)
{
	const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (k >= a.n_seqs) return;
	const int64_t seq = a.ids ? (int64_t)a.ids[k] : k;
	const int64_t b = a.limits[seq];
	const int64_t len = a.limits[seq + 1] - b - 1;
	if (len < SEG_WINDOW) return;                            // no window: the driver never looks at this sequence
	bool trigger = false;
	for (int64_t x = lane; x < len; x += 64) {
		int cls = SEG_NONE;
		if (x >= SEG_DOWNSET && x <= len - SEG_UPSET) {        // the window [x - 4, x + 5] lies inside the sequence
			int bogus;
			const int key = seg_window_key(a.data + b + x - SEG_DOWNSET, bogus);
			cls = seg_window_class(a.class_table, key, bogus);
		}
		a.cls[b + x] = (uint8_t)cls;
		trigger |= cls == SEG_TRIGGER;
	}
	if (__ballot(trigger) != 0 && lane == 0) a.work[atomicAdd(&a.counters[SEG_N_WORK], 1ull)] = (int32_t)seq;
}

// what seg_drive asks of a wavefront; every value it returns is the same in all lanes
struct WaveOps {
	const SegArgs& a;
	const int8_t* s;              // the sequence's letters
	const uint8_t* cls;           // ... and classes
	int seq, lane, n_emitted;
	int* comp;                    // LDS: composition of the raw segment
	uint8_t (*pre)[SEG_ALPHA];    // LDS: pre[k] = composition of its first k letters, suf[k] = of its last k letters
	uint8_t (*suf)[SEG_ALPHA];

	static __device__ bool passes(int c) { return c == SEG_TRIGGER || c == SEG_EXTEND; }
	__device__ int next_trigger(int i, int last) const
	{
		for (int x0 = i; x0 <= last; x0 += 64) {
			const int x = x0 + lane;
			const unsigned long long m = __ballot(x <= last && cls[x] == SEG_TRIGGER);
			if (m) return x0 + __ffsll(m) - 1;
		}
		return -1;
	}
	__device__ int find_high(int i, int last) const
	{
		for (int x0 = i; x0 <= last; x0 += 64) {
			const int x = x0 + lane;
			const unsigned long long m = __ballot(x <= last && !passes(cls[x]));
			if (m) return x0 + __ffsll(m) - 2;
		}
		return last;
	}
	__device__ int find_low(int i, int lowlim) const
	{
		for (int x0 = i; x0 >= lowlim; x0 -= 64) {
			const int x = x0 - lane;
			const unsigned long long m = __ballot(x >= lowlim && !passes(cls[x]));
			if (m) return x0 - __ffsll(m) + 2;
		}
		return lowlim;
	}
	__device__ bool trim(int left, int len, int& cut_left, int& cut_right) const
	{
		if (len > SEG_LNFACT_MAX) return false;
		const int8_t* r = s + left;
		__syncthreads();                                       // (one wavefront per workgroup) the previous trim's reads are done
		if (lane < SEG_ALPHA) comp[lane] = 0;
		__syncthreads();
		for (int x = lane; x < len; x += 64) { const int l = r[x] & 31; if (l < SEG_ALPHA) atomicAdd(&comp[l], 1); }
		const int dmax = len - 2 < SEG_MAX_TRIM - 1 ? len - 2 : SEG_MAX_TRIM - 1;
		if (lane < SEG_ALPHA) {                                // a lane per residue: running counts over the first dmax letters ...
			int n = 0;
			for (int k = 0; k <= dmax; ++k) { pre[k][lane] = (uint8_t)n; n += (r[k] & 31) == lane; }
		}
		else if (lane >= 32 && lane < 32 + SEG_ALPHA) {        // ... and over the last
			int n = 0;
			for (int k = 0; k <= dmax; ++k) { suf[k][lane - 32] = (uint8_t)n; n += (r[len - 1 - k] & 31) == lane - 32; }
		}
		__syncthreads();
		const int n_cand = seg_candidates(len);
		double best_v = 1.0;
		int best_c = 0x7fffffff;
		for (int c0 = 0; c0 < n_cand; c0 += 64) {
			double v = 1.0;
			int c = 0x7fffffff;
			if (c0 + lane < n_cand) {
				c = c0 + lane;
				int d, i, sv[SEG_ALPHA];
				seg_candidate(c, d, i);
				const uint32_t* p = reinterpret_cast<const uint32_t*>(pre[i]);
				const uint32_t* q = reinterpret_cast<const uint32_t*>(suf[d - i]);
#pragma unroll
				for (int w = 0; w < SEG_ALPHA / 4; ++w) {
					const uint32_t pw = p[w], qw = q[w];
#pragma unroll
					for (int j = 0; j < 4; ++j) sv[4 * w + j] = comp[4 * w + j] - (int)((pw >> (8 * j)) & 255) - (int)((qw >> (8 * j)) & 255);
				}
				seg_sort_desc(sv);
				v = seg_ln_prob(sv, len - d, a.lnfact);
			}
#pragma unroll
			for (int m = 32; m >= 1; m >>= 1) {
				const double ov = __shfl_xor(v, m);
				const int oc = __shfl_xor(c, m);
				if (seg_better(ov, oc, v, c)) { v = ov; c = oc; }
			}
			if (v < 1.0 && seg_better(v, c, best_v, best_c)) { best_v = v; best_c = c; }
		}
		cut_left = cut_right = 0;
		if (best_v < 1.0) {
			int d, i;
			seg_candidate(__builtin_amdgcn_readfirstlane(best_c), d, i);
			cut_left = i; cut_right = d - i;
		}
		return true;
	}
	__device__ void emit(int begin, int end)
	{
		if (lane == 0) {
			const unsigned long long slot = atomicAdd(&a.counters[SEG_N_RANGES], 1ull);
			if (slot < a.range_cap) a.ranges[slot] = SegRange{ seq, n_emitted, begin, end };
		}
		++n_emitted;
	}
	__device__ void remainder_done(int) const {}
};

__global__ __launch_bounds__(64) void seg_segments_kernel(const SegArgs a, int64_t n_work)
{
	__shared__ int comp[SEG_ALPHA];
	__shared__ __attribute__((aligned(4))) uint8_t pre[SEG_MAX_TRIM][SEG_ALPHA];
	__shared__ __attribute__((aligned(4))) uint8_t suf[SEG_MAX_TRIM][SEG_ALPHA];
	const int64_t k = blockIdx.x;
	if (k >= n_work) return;
	const int seq = a.work[k];
	const int64_t b = a.limits[seq];
	const int len = (int)(a.limits[seq + 1] - b - 1);
	WaveOps ops{ a, a.data + b, a.cls + b, seq, (int)threadIdx.x, 0, comp, pre, suf };
	// a sequence that is handed back may have left ranges in the list: the host drops them with the sequence
	if (!seg_drive(ops, len) && threadIdx.x == 0) a.handed[atomicAdd(&a.counters[SEG_N_HANDED], 1ull)] = seq;
}

__global__ __launch_bounds__(256) void seg_apply_kernel(const SegArgs a, int64_t n_ranges)
{
	const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (k >= n_ranges) return;
	const SegRange r = a.ranges[k];
	int8_t* s = a.data + a.limits[r.seq];
	for (int x = r.begin + lane; x <= r.end; x += 64) s[x] = 23;
}

}  // namespace

hipError_t launch_seg_classes(const SegArgs& a, hipStream_t st)
{
	if (a.n_seqs <= 0) return hipSuccess;
	seg_class_kernel<<<dim3((unsigned)((a.n_seqs + 3) / 4)), dim3(256), 0, st>>>(a);
	return hipGetLastError();
}

hipError_t launch_seg_segments(const SegArgs& a, int64_t n_work, hipStream_t st)
{
	if (n_work <= 0) return hipSuccess;
	seg_segments_kernel<<<dim3((unsigned)n_work), dim3(64), 0, st>>>(a, n_work);
	return hipGetLastError();
}

hipError_t launch_seg_apply(const SegArgs& a, int64_t n_ranges, hipStream_t st)
{
	if (n_ranges <= 0) return hipSuccess;
	seg_apply_kernel<<<dim3((unsigned)((n_ranges + 3) / 4)), dim3(256), 0, st>>>(a, n_ranges);
	return hipGetLastError();
}

}  // namespace dmnd
