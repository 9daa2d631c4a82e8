// tests/emu/xdrop_emu.cpp -- TEST INFRASTRUCTURE ONLY. The host instantiation of the x-drop walk the device kernel shares with the
// host's chaining stage (diamond_amd/csrc/xdrop_core.h), called the way xdrop_seg_kernel calls it: the left walk from qa - 1 / sa - 1
// with best 0, then the right walk from qa / sa with the left walk's result.
#include "../../diamond_amd/csrc/xdrop_core.h"

// one direction: returns the best sum, *reach = letters up to it
extern "C" int emu_xdrop_walk(const int8_t* M, const int8_t* q, const int8_t* cbs, const int8_t* t, int dir, int best, int xdrop, int* reach)
{
	return dmnd::xdrop_walk_core<int8_t>(M, q, cbs, t, dir, best, xdrop, *reach);
}

// both walks of n seed hits (qa: offset into the query block, sa: offset into the target block); out: left, right, score per hit
extern "C" void emu_xdrop_segments(const int8_t* M, const int8_t* qblock, const int8_t* cbs, const int8_t* tblock, const int64_t* qa, const int64_t* sa,
	int64_t n, int xdrop, int32_t* out)
{
	for (int64_t k = 0; k < n; ++k) {
		const int8_t* q = qblock + qa[k];
		const int8_t* t = tblock + sa[k];
		const int8_t* c = cbs ? cbs + qa[k] : nullptr;
		int left, right;
		const int s_left = dmnd::xdrop_walk_core<int8_t>(M, q - 1, c ? c - 1 : nullptr, t - 1, -1, 0, xdrop, left);
		const int s_both = dmnd::xdrop_walk_core<int8_t>(M, q, c, t, +1, s_left, xdrop, right);
		out[3 * k] = left; out[3 * k + 1] = right; out[3 * k + 2] = s_both;
	}
}
