// tuning.h -- the library's tuning values in ONE place (round 6; the round-5 review counted 51 getenv calls scattered over csrc/).
// None of them is part of the ABI; every one has a measured default and is read ONCE per process from the environment variable
// named beside it (the sweeps that chose the defaults: DESIGN.md 6.4, 6.6, 4.17; tools/seed_modes.py).
// Not here, on purpose: diagnostics (DMND_TRACE*, DMND_SEED_PHASES, DMND_CLI_TIMELINE), the tests' hooks that force a rare path
// per call (DMND_TRACE_ARENA_MB, DMND_SWIPE32 ...; those of the seed search -- DMND_SEED_CHAIN / _TILED / _CLASSES_LONG / _SLICES /
// _SLICES_BUDGET_MB / _SLICES_MIN_LETTERS / _SLICE_WORDS, the buffer caps _MATCHED_CAP / _SURVIVOR_CAP / _HIT_CAP / _DEFERRED_CAP,
// _SORT_CAP, _READBACK_BYTES -- are read once per call in their own ONE place, seed_api.hip seed_hooks; DMND_SEED_FUSED in seed_sizes)
// and the A/B switches that keep the previous form of a stage alive as the second implementation parity tests compare with
// (DMND_EXTEND_DEVICE, _PLAN_GPU, _XDROP_GPU, _KEEP_TRACE): DESIGN.md 9 lists them all.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace dmnd {

struct Tuning {
	// ---- host waits (api.hip sync_stream / wait_event)
	bool spin_sync = false;            // DMND_SPIN_SYNC=1: the runtime's spinning waits (lowest latency, a core per waiting thread)
	int sync_spin_us = 150;            // DMND_SYNC_SPIN_US: busy poll before the sleeping poll (a short kernel's count is back by then)
	// ---- host worker pool (host_pool.h)
	int pool_spins = 600;              // DMND_POOL_SPINS: pause iterations a worker spins for the next loop before it sleeps
	// ---- thread layout of the extension's HOST path (extend_host.hip; the device half has no host threads)
	int extend_team = 8;               // DMND_EXTEND_TEAM: fixed host slices per call
	int extend_split = 1;              // DMND_EXTEND_SPLIT: sub-batches with their own streams (the layout of rounds 2-3), 1 = one range
	int extend_runners = 1;            // DMND_EXTEND_RUNNERS
	int extend_sub_threads = 0;        // DMND_EXTEND_SUB_THREADS: 0 = by the hits per runner
	// ---- sweeps (api.hip sweep_rows_min_items)
	int sweep_rows_min_items = 1 << 17; // DMND_SWEEP_ROWS_MIN: items of a launch set from which on bands of <= 96 / 160 diagonals take the row classes
	int extend_resweep_below_pct = 40; // DMND_EXTEND_RESWEEP_BELOW_PCT: device half: an iteration of which at most this share of the targets can survive the culling is swept for scores only, its survivors again with traceback (0 = always keep trace rows)
	// ---- streams
	bool no_stream_priority = false;   // DMND_NO_STREAM_PRIORITY: every stream at the default priority
	// ---- seed stage geometry (seed_api.hip seed_sizes; 0 = the size-dependent default chosen there)
	int seed_slots_x8 = 0;             // DMND_SEED_SLOTS_X8: table slots per query position x 8 (8 .. 64; default 32 fused / 16)
	// ---- chain mode of the long-seed search (seed_chain.h)
	// (values only: the environment variables of these two are the tests' per-call hooks, read in ONE place, seed_api.hip seed_hooks)
	int seed_readback_bytes = 1 << 20; // DMND_SEED_READBACK_BYTES: most bytes of sorted hits that come back with the chain's one copy
	// ---- sliced long-seed stream (seed_slices_core.h)
	// (values only, like the two above: their environment variables are per-call hooks read in seed_api.hip seed_hooks)
	// (no value for the size of the level-1 filter: a search on the sliced stream takes the largest the slices hold -- seed_slices_filter_words,
	// C2: 8 MB in 64 slices of 128 KB instead of the plain stream's L2-bound 3 MB; stream kernel 0.72 / 0.64 / 0.59 ms at 3 / 4 / 8 MB --,
	// DMND_SEED_SLICES_FILTER_WORDS is the per-call hook of tests and size sweeps)
	int seed_slices_budget_mb = 3072;  // DMND_SEED_SLICES_BUDGET_MB: most MB of reference-side cache a context keeps. 8 bytes per reference letter and shape (list entry and hash) plus half a byte per letter: C2's 3.0e8-letter block takes 2 561 397 480 bytes (2443 MB) with one shape; with the two of the default sensitivity it would take 4742 MB, which is over the budget, and such a search takes the plain stream (before the hashes two shapes fit, at 2439 MB; the budget was not raised: nothing measured asks for it). Only what is kept counts: the build's scratch (two routing bytes per window, the flag words, the radix pass's: about 0.7 GB more for C2's block until the build is done) does not, and a context that cannot allocate it takes the plain stream
	long long seed_slices_min_letters = 1 << 20;   // DMND_SEED_SLICES_MIN_LETTERS: reference block length from which on a repeated search takes the sliced stream (C2's query block: sliced / plain stream kernel 0.0179 / 0.0192 ms at 3e5 letters, 0.0189 / 0.0225 ms at 9e5, 0.287 / 0.453 ms at 9e7)
	long long seed_slices_max_joined = 1 << 20;    // (no hook) joined reference positions of the context's last search above which the default rule leaves the sliced stream out: C2skew (over 1.6e6 per step) ran 28.7 ms per step with it, 26.8-27.4 without, C2 (9e4) 2.50 against 2.98
	int seed_sort_cap = 1 << 16;       // DMND_SEED_SORT_CAP: entries of the padded sort whose size only the device knows (C2: 2e4 hits per step)
};

inline const Tuning& tuning()
{
	static const Tuning t = [] {
		Tuning x;
		auto num = [](const char* name, int fallback) { const char* e = std::getenv(name); return e ? std::atoi(e) : fallback; };
		{ const char* e = std::getenv("DMND_SPIN_SYNC"); x.spin_sync = e && e[0] == '1'; }
		x.sync_spin_us = std::max(0, num("DMND_SYNC_SPIN_US", x.sync_spin_us));
		x.pool_spins = std::max(0, num("DMND_POOL_SPINS", x.pool_spins));
		x.extend_team = std::max(1, num("DMND_EXTEND_TEAM", x.extend_team));
		x.extend_split = std::max(1, std::min(64, num("DMND_EXTEND_SPLIT", x.extend_split)));
		x.extend_runners = std::max(1, num("DMND_EXTEND_RUNNERS", x.extend_runners));
		x.extend_sub_threads = std::max(0, num("DMND_EXTEND_SUB_THREADS", x.extend_sub_threads));
		x.sweep_rows_min_items = std::max(0, num("DMND_SWEEP_ROWS_MIN", x.sweep_rows_min_items));
		x.extend_resweep_below_pct = std::max(0, std::min(100, num("DMND_EXTEND_RESWEEP_BELOW_PCT", x.extend_resweep_below_pct)));
		x.no_stream_priority = std::getenv("DMND_NO_STREAM_PRIORITY") != nullptr;
		if (std::getenv("DMND_SEED_SLOTS_X8")) x.seed_slots_x8 = std::min(64, std::max(8, num("DMND_SEED_SLOTS_X8", 0)));
		return x;
	}();
	return t;
}

}  // namespace dmnd
