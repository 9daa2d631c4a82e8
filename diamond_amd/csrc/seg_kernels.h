// seg_kernels.h -- launch interface of the SEG masking kernels (seg_kernels.hip; arithmetic in seg_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seg_core.h"

namespace dmnd {

struct SegRange { int32_t seq, order, begin, end; };      // segment [begin, end] (inclusive) of block sequence seq, the order-th of its list

enum { SEG_N_WORK = 0, SEG_N_RANGES = 1, SEG_N_HANDED = 2, SEG_COUNTERS = 4 };

struct SegArgs {
	int8_t* data;                 // block letters (HBM); only seg_apply_kernel writes them
	const int64_t* limits;        // sequence i = data[limits[i], limits[i+1] - 1)
	int64_t n_seqs;               // sequences of the call: the whole block, or the entries of ids
	const int32_t* ids;           // optional: only these sequences (block sequence ids)
	uint8_t* cls;                 // scratch, indexed like data: the class of the window centred at a letter
	const uint8_t* class_table;   // SEG_CLASS_TABLE classes by window key (built on the host from seg::entropy)
	const double* lnfact;         // ln n!, n = 0 .. SEG_LNFACT_MAX
	int32_t* work;                // out: the sequences that hold a trigger window (n_seqs entries), in no particular order
	int32_t* handed;              // out: the sequences the host has to redo (n_seqs entries)
	SegRange* ranges;             // out: range_cap entries, in no particular order
	unsigned long long range_cap;
	unsigned long long* counters; // SEG_N_WORK, SEG_N_RANGES (keeps counting above range_cap), SEG_N_HANDED
};

hipError_t launch_seg_classes(const SegArgs& a, hipStream_t st);
hipError_t launch_seg_segments(const SegArgs& a, int64_t n_work, hipStream_t st);
hipError_t launch_seg_apply(const SegArgs& a, int64_t n_ranges, hipStream_t st);

}  // namespace dmnd
