// seed_api.hip -- host side of the seed stage (include/diamond_hip.h: dmnd_seed_search / dmnd_seed_hits).
// Orchestrates seed_kernels.hip per shape: index queries -> stream the reference -> complexity masks (all shapes
// first, because a pair's left-most test needs the mask times of every earlier shape/chunk), then the pair filter
// per shape. Replaces the control flow of Search::search_shape (/root/reference/src/search/stage0.cpp:101-217).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <vector>
#include <chrono>
#include "ctx.h"
#include "seed_core.h"
#include "seed_kernels.h"

using namespace dmnd;

enum { SEED_CLASSES_LONG_DEFAULT = 1 };      // C5 (100 000 queries, 16 MB level-1 filter): stream 3.0 -> 2.06 ms per 1.9e8-letter block, seed stage 33.2 -> 25.4 ms per 8 blocks (tools/gpu_r05b.sh)

static_assert(sizeof(dmnd_seed_params) == sizeof(SeedParams), "dmnd_seed_params must mirror dmnd::SeedParams");
static_assert(sizeof(dmnd_seed_hit) == 24, "dmnd_seed_hit layout");

extern "C" int dmnd_seed_params_fast(dmnd_seed_params* p, int threads)
{
	if (!p || threads < 1) return fail(DMND_E_ARG, "dmnd_seed_params_fast: bad argument");
	std::memset(p, 0, sizeof(*p));
	const char* code = "1101110101101111";                 // shape_codes[FAST], search/setup.cpp:211-212
	p->n_shapes = 1;
	int w = 0, len = (int)std::strlen(code);
	for (int i = 0; i < len; ++i)
		if (code[i] == '1') { p->shape_pos[0][w++] = (int8_t)i; p->shape_mask[0] |= 1u << i; }
	p->shape_len[0] = len; p->shape_weight[0] = w;
	// murphy10 "A KR EDNQ C G H ILVM FYW P ST" over ARNDCQEGHILKMFPSTWYV (stats/stats.cpp:48, basic/value.h:53);
	// X and '*' reduce to the mask letter, every other code to class 0 (Reduction ctor, basic.cpp:267-297)
	static const int8_t murphy10[32] = { 0, 1, 2, 2, 3, 2, 2, 4, 5, 6, 6, 1, 6, 7, 8, 9, 9, 7, 7, 6, 0, 0, 0, 23, 23, 0, 0, 0, 0, 0, 0, 0 };
	std::memcpy(p->reduction, murphy10, 32);
	p->reduction_size = 10;
	p->index_chunks = 4;                                    // sensitivity_traits[FAST].index_chunks
	p->hamming_filter_id = 11;
	// seedp_bits(): max(bit_length(size^weight - 1) - 32, bit_length(threads*4*chunks - 1), 8), setup.cpp:306-309
	auto bit_length = [](uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; };
	uint64_t space = 1;
	for (int i = 0; i < w; ++i) space *= 10;
	p->seedp_bits = std::max(std::max(bit_length(space - 1) - 32, bit_length((uint64_t)threads * 4 * p->index_chunks - 1)), 8);
	p->ungapped_window = 48;
	p->left_most_interval = 32;
	p->seed_complexity_cut = 0.9 * 0.69314718055994530942 * w;      // seed_cut * log(2) * weight, setup.cpp:369-370
	p->use_ungapped = 0; p->short_query_max_len = 60; p->tile_size = 1024; p->simd_lanes = 32;
	return DMND_OK;
}

namespace {

// shapes + the stage-2 ungapped e-value filter (10000) shared by the default and sensitive presets
int spaced_preset(dmnd_seed_params* p, int threads, const dmnd_params* sc, const char* const* codes, int n, double seed_cut,
	double ungapped_evalue = 10000.0, double ungapped_evalue_short = 10000.0, int hamming_id = 11, int index_chunks = 4)
{
	if (int rc = dmnd_seed_params_fast(p, threads)) return rc;
	p->n_shapes = n;
	p->hamming_filter_id = hamming_id;
	p->index_chunks = index_chunks;
	int weight = 0;
	for (int sid = 0; sid < n; ++sid) {
		int w = 0;
		const int len = (int)std::strlen(codes[sid]);
		p->shape_mask[sid] = 0;
		std::memset(p->shape_pos[sid], 0, sizeof(p->shape_pos[sid]));
		for (int i = 0; i < len; ++i)
			if (codes[sid][i] == '1') { p->shape_pos[sid][w++] = (int8_t)i; p->shape_mask[sid] |= 1u << i; }
		p->shape_len[sid] = len; p->shape_weight[sid] = w;
		weight = w;
	}
	auto bit_length = [](uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; };
	uint64_t space = 1;
	for (int i = 0; i < weight; ++i) space *= (uint64_t)p->reduction_size;
	p->seedp_bits = std::max(std::max(bit_length(space - 1) - 32, bit_length((uint64_t)threads * 4 * p->index_chunks - 1)), 8);      // setup.cpp:306-309
	p->seed_complexity_cut = seed_cut * 0.69314718055994530942 * weight;       // setup.cpp:369-370
	// ungapped e-value 10000: CutoffTable + short-query cutoff (cutoff_table.h:30-35, score_matrix.h:130-151, config.cpp:431)
	const double LN2 = 0.69314718055994530941723212145818, ln_k = std::log(sc->K);
	auto raw = [&](double bits) { return (int32_t)std::ceil((bits * LN2 + ln_k) / sc->lambda); };
	p->use_ungapped = 1;
	p->short_query_cutoff = raw(25.0);
	p->cutoff_table[0] = 0;
	p->cutoff_table_short[0] = 0;
	for (int b = 1; b < 32; ++b) {
		p->cutoff_table[b] = raw(-std::log(ungapped_evalue / 1e9 / (double)(1u << (b - 1))) / std::log(2.0));
		p->cutoff_table_short[b] = raw(-std::log(ungapped_evalue_short / 1e9 / (double)(1u << (b - 1))) / std::log(2.0));
	}
	return DMND_OK;
}

}

extern "C" int dmnd_seed_params_default(dmnd_seed_params* p, int threads, const dmnd_params* sc)
{
	if (!p || !sc || threads < 1) return fail(DMND_E_ARG, "dmnd_seed_params_default: bad argument");
	static const char* const codes[2] = { "111101110111", "111011010010111" };          // shape_codes[DEFAULT], search/setup.cpp:82-84
	return spaced_preset(p, threads, sc, codes, 2, 0.8);
}

extern "C" int dmnd_seed_params_sensitive(dmnd_seed_params* p, int threads, const dmnd_params* sc)
{
	if (!p || !sc || threads < 1) return fail(DMND_E_ARG, "dmnd_seed_params_sensitive: bad argument");
	static const char* const codes[16] = {                                               // shape_codes[SENSITIVE], search/setup.cpp:86-102
		"1011110111", "110100100010111", "11001011111", "101110001111", "11011101100001", "1111010010101", "111001001001011",
		"10101001101011", "111101010011", "1111000010000111", "1100011011011", "1101010000011011", "1110001010101001",
		"110011000110011", "11011010001101", "1101001100010011" };
	return spaced_preset(p, threads, sc, codes, 16, 1.0);
}

// One entry for every sensitivity this library presets: shape set, seed cut and the gapped-filter e-value that goes with it
// (sensitivity_traits + shape_codes, search/setup.cpp:40-53,80-215)
extern "C" int dmnd_seed_params_preset(dmnd_seed_params* p, int sensitivity, int threads, const dmnd_params* sc, double* gapped_filter_evalue)
{
	if (!p || threads < 1) return fail(DMND_E_ARG, "dmnd_seed_params_preset: bad argument");
	if (gapped_filter_evalue) *gapped_filter_evalue = 0.0;
	switch (sensitivity) {
	case DMND_SENS_FAST: return dmnd_seed_params_fast(p, threads);
	case DMND_SENS_DEFAULT: return dmnd_seed_params_default(p, threads, sc);
	case DMND_SENS_MID_SENSITIVE: {
		if (!sc) return fail(DMND_E_ARG, "dmnd_seed_params_preset: scoring parameters needed");
		static const char* const codes[8] = { "11110110111", "1101100111101", "1110010101111", "11010101100111", "11101110001011",
			"1110100100010111", "1101000011010111", "1110011000011011" };                   // 8x9, setup.cpp:196-205
		return spaced_preset(p, threads, sc, codes, 8, 1.0);
	}
	case DMND_SENS_SENSITIVE:
	case DMND_SENS_MORE_SENSITIVE:       // same shapes and filters; differs only in freq_sd / motif masking, which this library does not apply
		if (gapped_filter_evalue) *gapped_filter_evalue = 1.0;
		return dmnd_seed_params_sensitive(p, threads, sc);
	case DMND_SENS_VERY_SENSITIVE: {
		if (!sc) return fail(DMND_E_ARG, "dmnd_seed_params_preset: scoring parameters needed");
		static const char* const codes[14] = { "11101111", "110110111", "111111001", "1010111011", "11110001011", "110100101011", "110110001101",
			"1010101000111", "1100101001011", "1101010101001", "1110010010011", "110110000010011", "111001000100011", "1101000100010011" };   // 14x7, setup.cpp:118-133
		if (gapped_filter_evalue) *gapped_filter_evalue = 1.0;
		// sensitivity_traits: min id 9, ungapped e-values 100000 / 30000 (short), one index chunk (setup.cpp:51)
		return spaced_preset(p, threads, sc, codes, 14, 1.0, 100000.0, 30000.0, 9, 1);
	}
	case DMND_SENS_ULTRA_SENSITIVE: {
		if (!sc) return fail(DMND_E_ARG, "dmnd_seed_params_preset: scoring parameters needed");
		static const char* const codes[64] = { "1111111", "11101111", "110011111", "110110111", "111111001", "1010111011", "1011110101", "1111000111",
			"10011110011", "10101101101", "10111010101", "11001010111", "11001100111", "11010101101", "11110001011", "100111010011", "101100110101",
			"101110000111", "110100101011", "110110001101", "111000110011", "1010001011011", "1010101000111", "1010110100011", "1100100110011",
			"1100101001011", "1101001100101", "1101010101001", "1110001010101", "1110010010011", "10100001101101", "11000100010111", "11010000100111",
			"11010100110001", "11101000011001", "11110000001101", "11110100000011", "101001000001111", "110000100101011", "110010010000111",
			"110101100001001", "110110000010011", "111001000100011", "111100000100101", "1000110010010101", "1001000100101101", "1001000110011001",
			"1010001001001011", "1010001010010011", "1010010001010101", "1010010100010011", "1010010101001001", "1010100000101011", "1010100011000101",
			"1011000010001011", "1100010000111001", "1100010010001011", "1100100001001011", "1100100100100011", "1100110000001101", "1101000100010011",
			"1101000110000101", "1110000001010011", "1110100000010101" };                                   // 64x7, setup.cpp:135-200
		if (gapped_filter_evalue) *gapped_filter_evalue = 1.0;
		// sensitivity_traits: min id 9, ungapped e-values 300000 / 30000 (short), one index chunk (setup.cpp:53)
		return spaced_preset(p, threads, sc, codes, 64, 1.0, 300000.0, 30000.0, 9, 1);
	}
	default:
		return fail(DMND_E_ARG, "dmnd_seed_params_preset: unknown sensitivity");
	}
}

extern "C" int dmnd_seed_params_set_index_chunks(dmnd_seed_params* p, int index_chunks, int threads)
{
	if (!p || index_chunks < 1 || threads < 1 || p->n_shapes < 1) return fail(DMND_E_ARG, "dmnd_seed_params_set_index_chunks: bad argument");
	auto bit_length = [](uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; };
	uint64_t space = 1;
	for (int i = 0; i < p->shape_weight[0]; ++i) space *= (uint64_t)p->reduction_size;
	p->index_chunks = index_chunks;
	p->seedp_bits = std::max(std::max(bit_length(space - 1) - 32, bit_length((uint64_t)threads * 4 * index_chunks - 1)), 8);      // setup.cpp:306-309
	return DMND_OK;
}

extern "C" int dmnd_seed_params_set_query_indexed(dmnd_seed_params* p, int threads)
{
	if (!p || threads < 1 || p->n_shapes < 1) return fail(DMND_E_ARG, "dmnd_seed_params_set_query_indexed: bad argument");
	if (p->reduction_size > 16) return fail(DMND_E_ARG, "dmnd_seed_params_set_query_indexed: the hashed seed encoding packs 4 bits per letter");
	for (int i = 0; i < p->n_shapes; ++i)
		if (p->shape_len[i] > 16) return fail(DMND_E_ARG, "dmnd_seed_params_set_query_indexed: shapes longer than 16 letters");
	p->seed_encoding = SEED_HASHED;
	return dmnd_seed_params_set_index_chunks(p, 1, threads);       // run/double_indexed.cpp:297: one index chunk unless -c is given
}

extern "C" int dmnd_auto_query_indexed(const dmnd_seed_params* params, const int8_t* qdata, const int64_t* qlimits, int64_t nq, int64_t db_bytes, int* query_indexed)
{
	if (!params || !qdata || !qlimits || nq < 0 || !query_indexed) return fail(DMND_E_ARG, "dmnd_auto_query_indexed: bad argument");
	*query_indexed = 0;
	const int64_t MiB = (int64_t)1 << 20;
	const int64_t letters = nq > 0 ? qlimits[nq] - qlimits[0] - nq : 0;
	if (letters > 32 * MiB || db_bytes < 256 * MiB) return DMND_OK;                    // MAX_INDEX_QUERY_SIZE, MIN_QUERY_INDEXED_DB_SIZE
	if (params->reduction_size > 16) return DMND_OK;
	for (int i = 0; i < params->n_shapes; ++i) if (params->shape_len[i] > 16) return DMND_OK;
	auto next_pow2 = [](double x) { uint64_t n = (uint64_t)std::ceil(x), p = 1; while (p < n) p <<= 1; return p; };
	// a shape has at most one seed per letter: only query blocks close to the 32 Mi limit need their seeds counted
	if (next_pow2((double)letters * 1.25) <= (uint64_t)(32 * MiB)) { *query_indexed = 1; return DMND_OK; }
	SeedParams sp;
	std::memcpy(&sp, params, sizeof(sp));
	sp.seed_encoding = SEED_HASHED;
	// (3e7 keys per shape for a block at the limit: sorted on one thread that was 2.3 s per shape, more than the whole search of
	// such a block takes on the device. Eight threads: each counts the seeds of its eighth of the sequences per key class, then
	// writes them into ONE array grouped by class -- huge pages asked for: 240 MB of first-touched 4 KB pages cost 0.9 s under
	// eight faulting threads --, then each sorts and counts one class in place)
	uint64_t largest = 0;
	constexpr int T = 8;
	const size_t cap = (size_t)letters + 16;
	const size_t bytes = ((cap * sizeof(uint64_t) + ((size_t)2 << 20) - 1) >> 21) << 21;
	uint64_t* keys = static_cast<uint64_t*>(std::aligned_alloc((size_t)2 << 20, bytes));
	if (!keys) return fail(DMND_E_NOMEM, "dmnd_auto_query_indexed: out of memory");
	(void)madvise(keys, bytes, MADV_HUGEPAGE);
	auto key_class = [](uint64_t k) { return (int)((k * 0x9E3779B97F4A7C15ull) >> 61); };
	for (int sid = 0; sid < sp.n_shapes; ++sid) {
		size_t count[T][T] = { { 0 } }, at[T][T];             // [producer][class]
		uint64_t distinct[T] = { 0 };
		auto for_seeds = [&](int t, auto&& f) {
			for (int64_t i = nq * t / T; i < nq * (t + 1) / T; ++i)
				for (int64_t p = qlimits[i]; p + sp.shape_len[sid] < qlimits[i + 1]; ++p) {
					uint64_t k;
					if (seed_key_hashed(sp, sid, qdata + p, k)) f(k);
				}
		};
		auto team = [&](auto&& body) {
			std::vector<std::thread> th;
			for (int t = 0; t < T; ++t) th.emplace_back([&, t] { body(t); });
			for (std::thread& x : th) x.join();
		};
		team([&](int t) { for_seeds(t, [&](uint64_t k) { ++count[t][key_class(k)]; }); });
		size_t class_begin[T + 1], off = 0;
		for (int c = 0; c < T; ++c) { class_begin[c] = off; for (int t = 0; t < T; ++t) { at[t][c] = off; off += count[t][c]; } }
		class_begin[T] = off;
		team([&](int t) { for_seeds(t, [&](uint64_t k) { keys[at[t][key_class(k)]++] = k; }); });
		team([&](int c) {
			std::sort(keys + class_begin[c], keys + class_begin[c + 1]);
			distinct[c] = (uint64_t)(std::unique(keys + class_begin[c], keys + class_begin[c + 1]) - (keys + class_begin[c]));
		});
		uint64_t all = 0;
		for (int c = 0; c < T; ++c) all += distinct[c];
		largest = std::max(largest, next_pow2((double)all * 1.25));
		if (largest > (uint64_t)(32 * MiB)) break;          // the answer is no whatever the other shapes say
	}
	std::free(keys);
	*query_indexed = largest <= (uint64_t)(32 * MiB) ? 1 : 0;
	return DMND_OK;
}

extern "C" int dmnd_set_query_index_reuse(dmnd_ctx* c, int on)
{
	if (!c) return fail(DMND_E_ARG, "dmnd_set_query_index_reuse: ctx is NULL");
	c->reuse_query_index = on != 0;
	c->qindex_signature.clear();
	return DMND_OK;
}

extern "C" int dmnd_set_min_length_ratio(dmnd_ctx* c, double ratio)
{
	if (!c) return fail(DMND_E_ARG, "dmnd_set_min_length_ratio: ctx is NULL");
	if (!(ratio >= 0.0 && ratio <= 1.0)) return fail(DMND_E_ARG, "dmnd_set_min_length_ratio: the ratio lies in [0, 1]");
	c->min_length_ratio = ratio;
	return DMND_OK;
}

extern "C" int dmnd_set_linsearch(dmnd_ctx* c, int on)
{
	if (!c) return fail(DMND_E_ARG, "dmnd_set_linsearch: ctx is NULL");
	c->linsearch = on != 0;
	return DMND_OK;
}

extern "C" int dmnd_length_sort_order(const int64_t* limits, int64_t n, int64_t* order)
{
	if (n < 0 || (n > 0 && (!limits || !order))) return fail(DMND_E_ARG, "dmnd_length_sort_order: bad argument");
	length_sort_order(limits, n, order);
	return DMND_OK;
}

extern "C" int dmnd_seed_query_windows(dmnd_ctx* c, uint32_t* out, int64_t n_targets)
{
	if (!c || !out) return fail(DMND_E_ARG, "dmnd_seed_query_windows: NULL argument");
	if (c->seed_qwin_n <= 0 || n_targets != c->seed_qwin_n) return fail(DMND_E_ARG, "dmnd_seed_query_windows: the last seed search built no windows for that many targets");
	HIP_TRY(hipSetDevice(c->device));
	static_assert(sizeof(SeedQueryWindow) == 2 * sizeof(uint32_t), "two words per window");
	return download_bytes(c, out, c->seed_qwin.p, (size_t)n_targets * sizeof(SeedQueryWindow));
}

extern "C" int dmnd_seed_kernel_ms(const dmnd_ctx* c, double ms[5])
{
	if (!c || !ms) return fail(DMND_E_ARG, "dmnd_seed_kernel_ms: bad argument");
	for (int i = 0; i < 5; ++i) ms[i] = c->seed_ms[i];
	return DMND_OK;
}

namespace {

// Device time of the phases of a search (dmnd_seed_kernel_ms), WITHOUT a host wait per phase: start / stop only record events on
// the stream, collect() reads every pair once the search has been waited for anyway. (Until round 5 stop() waited for its event:
// four host round trips per shape that served nothing but the clock -- an interrupt-driven wake-up and an idle device each,
// ~0.13 ms of the 2.46 ms a C2 seed stage takes.)
struct Timer {
	hipStream_t st;
	hipEvent_t open = nullptr;
	struct Span { hipEvent_t a, b; double* into; };
	std::vector<Span> spans;
	Timer(hipStream_t s) : st(s) {}
	~Timer() { if (open) (void)hipEventDestroy(open); for (const Span& x : spans) { (void)hipEventDestroy(x.a); (void)hipEventDestroy(x.b); } }
	void start()
	{
		if (!open) (void)hipEventCreate(&open);
		(void)hipEventRecord(open, st);
	}
	void stop(double& into)
	{
		if (!open) return;
		hipEvent_t b = nullptr;
		(void)hipEventCreateWithFlags(&b, spin_sync() ? hipEventDefault : hipEventBlockingSync);
		(void)hipEventRecord(b, st);
		spans.push_back(Span{ open, b, &into });
		open = nullptr;
	}
	// a phase that runs again after an overflow: the spans of the abandoned attempt do not count
	void discard(const double* into)
	{
		size_t k = 0;
		for (const Span& x : spans)
			if (x.into == into) { (void)hipEventDestroy(x.a); (void)hipEventDestroy(x.b); }
			else spans[k++] = x;
		spans.resize(k);
	}
	void collect()
	{
		if (!spans.empty()) (void)wait_event(spans.back().b);
		for (const Span& x : spans) {
			float ms = 0;
			if (hipEventElapsedTime(&ms, x.a, x.b) == hipSuccess) *x.into += ms;
			(void)hipEventDestroy(x.a); (void)hipEventDestroy(x.b);
		}
		spans.clear();
	}
};

}

// Buffer geometry of a seed search: a function of the seed parameters and the number of query positions only, so that the buffers
// can be reserved (dmnd_seed_reserve) before the blocks are resident
struct SeedSizes {
	uint64_t slots, bm_words, bm1_words;
	uint32_t bm1_k3;
	int SB, slot_shift;
	bool fused, reuse;
	size_t bm_total;
};

static SeedSizes seed_sizes(const dmnd_ctx* c, const SeedParams& sp, int64_t nq_pos)
{
	SeedSizes z;
	const int S = sp.n_shapes;
	// Table slots per query position: two for long seeds, FOUR for the short seeds of the fused pipeline, where a third of the
	// reference positions probe the table and the probe chains are what costs (most query seeds are distinct: two slots per
	// position = 36 % load). Measured on C3 (16 shapes): stream + filter 189 / 124 / 116 / 115 ms at 1 / 2 / 4 / 8 slots per position
	// (DMND_SEED_SLOTS_X8 = 8 / 16 / 32 / 64, slots per position in eighths).
	const uint64_t slots_x8 = (uint64_t)(tuning().seed_slots_x8 ? tuning().seed_slots_x8 : (seed_stream_can_fuse(sp) ? 32 : 16));
	z.slots = 1024;
	while (z.slots * 8 < (uint64_t)nq_pos * slots_x8) z.slots <<= 1;
	// slot numbers are 32-bit in the position lists and the joined-position records (LIST_END = all ones): a query block above 2^30
	// positions keeps the table at 2^31 slots, i.e. fewer slots per position (the query-block limit of 4 G letters is checked by the caller)
	while (z.slots > ((uint64_t)1 << 31) && z.slots / 2 >= (uint64_t)nq_pos + (uint64_t)nq_pos / 4) z.slots >>= 1;

	// bitmap: >= 16 bits per query position, at most 2^27 bits (16 MB); word mask for 32-bit words
	uint64_t bm_words = 1 << 15;
	while (bm_words * 32 < (uint64_t)nq_pos * 16 && bm_words < ((uint64_t)1 << 22)) bm_words <<= 1;
	// level-1 bitmap: 2^24 bits = 2 MB by default (half an XCD's L2), never larger than level 2
	// ... unless the query block is so large that 2 MB saturate (above 16 M positions more than 85 % of the bits are set and nearly
	// every probe is positive): then 4 bits per position, up to 2^27 -- a filter that works from the Infinity Cache beats one in
	// L2 that does not filter (100k queries: stream 34 -> 24 ms per 8 blocks). Below that the L2-resident size wins even at 70 %
	// density (blastx, 10 M positions: 3.7 against 5.8 ms).
	int bm1_log2 = 24;
	if (nq_pos > ((int64_t)1 << 24))
		while (bm1_log2 < 27 && ((uint64_t)1 << bm1_log2) < (uint64_t)nq_pos * 4) ++bm1_log2;
	uint64_t bm1_words = ((uint64_t)1 << bm1_log2) / 32;
	if (bm1_words > bm_words) bm1_words = bm_words;
	uint32_t bm1_k3 = 0;
	// Long seeds (level-2 path: nearly every level-1 positive is a false one) with a query block that the default size serves:
	// 3 MB and three bits per seed. Measured on C2 (3e6 query seeds): the stream kernel takes the same
	// 1.45 ms as with 2 MB / two bits -- its bound is the rate at which the L2s serve 4-byte probes, not the misses behind
	// them -- but the false positives drop from 9.7 % to 3.1 %, and with them the level-2 / table lines fetched over the fabric
	// (4 MB: 1.53 ms, 8 MB: 2.56 ms -- the PLAIN stream's filter has to fit an XCD's 4 MB L2 beside the stream. The sliced stream
	// probes from LDS and is not bound by L2: a search that takes it sizes its filter by seed_sizes_sliced below.)
	const bool long_seeds = !seed_stream_can_fuse(sp);
	if (long_seeds && bm1_log2 == 24 && bm_words >= 3 * bm1_words / 2) {
		bm1_words = 3 * bm1_words / 2;
		bm1_k3 = (uint64_t)nq_pos * 4 <= bm1_words * 32 ? 1u : 0u;      // a third bit pays from ~4.3 filter bits per seed up (optimum k = ln 2 x bits per seed)
	}
	// Short seeds by class (round 5 sweep on C3, tools/gpu_r05b.sh): 4 MB / three bits -- half a megabyte per XCD -- instead of 2 MB / two:
	// stream + filter 103.9 -> 102.6 ms per 16 shapes (8 MB: 103.4; fewer false positives = fewer slot lines fetched over the fabric)
	if (!long_seeds && bm1_log2 == 24 && bm_words >= 2 * bm1_words) { bm1_words *= 2; bm1_k3 = 1u; }
	// The fused pipeline finishes a shape before it starts the next one: its table, lists and bitmaps are ONE shape's, reused
	// (64 shapes of --ultra-sensitive would otherwise hold 8 GB of tables for a 10k-query block)
	bool fused = seed_stream_can_fuse(sp);
	if (const char* e = getenv("DMND_SEED_FUSED")) fused = fused && atoi(e) != 0;
	// Query index reuse (dmnd_set_query_index_reuse; a query block against many reference blocks): the tables, lists and bitmaps of
	// ALL shapes stay resident between calls and a call that finds them built for the same query block and parameters only resets
	// the per-block state (join / erase marks) instead of rebuilding them. Needs S buffer sets; refused above 64 GiB.
	z.slot_shift = 4;
	const size_t set_bytes = (z.slots << z.slot_shift) + 2 * (size_t)nq_pos * sizeof(uint32_t) + (size_t)(bm_words + bm1_words) * sizeof(uint32_t);
	const bool reuse = c->reuse_query_index && set_bytes * (size_t)S <= ((size_t)64 << 30) && !getenv("DMND_SEED_MATCHED_CAP");
	const int SB = (fused && !reuse) ? 1 : S;            // shapes that own buffers at the same time
	const size_t bm_total = (size_t)SB * (bm_words + bm1_words) * sizeof(uint32_t);
	z.bm_words = bm_words; z.bm1_words = bm1_words; z.bm1_k3 = bm1_k3;
	z.fused = fused; z.reuse = reuse; z.SB = SB; z.bm_total = bm_total;
	return z;
}

// The geometry of the same search on the sliced stream (seed_slices_filter_words: a level-1 filter sized for LDS slices, not for L2),
// or z itself where the search keeps seed_sizes' filter on either stream: the fused pipeline, hashed seeds, a query block above
// 2^24 positions (seed_sizes' own larger filters, probed by key class), a kept query index (one index serves reference blocks that
// may take different streams), a size that finds no slice count. slice_words / forced_words: SeedHooks.
static SeedSizes seed_sizes_sliced(const dmnd_ctx* c, const SeedParams& sp, int64_t nq_pos, const SeedSizes& z, uint32_t slice_words, uint64_t forced_words)
{
	if (z.fused || seed_stream_can_fuse(sp) || sp.seed_encoding != SEED_SPACED || nq_pos > ((int64_t)1 << 24) || c->reuse_query_index) return z;
	int slot_bits = 0;
	while (((uint64_t)1 << slot_bits) < z.slots) ++slot_bits;
	SeedSizes s = z;
	s.bm1_words = seed_slices_filter_words((uint64_t)nq_pos, slot_bits, z.bm_words, z.bm1_words, slice_words, forced_words, &s.bm1_k3);
	s.bm_total = (size_t)s.SB * (s.bm_words + s.bm1_words) * sizeof(uint32_t);
	return s;
}

// The buffers a search of this geometry needs before its first kernel. generous: also the buffers whose size depends on what the
// search finds, at their starting capacities (dmnd_seed_reserve; the search itself grows them where they overflow)
// bitmap_bytes: the filters of the geometry or of its sliced form (seed_sizes_sliced), whichever are larger -- the searches of one
// reference block take either
static int seed_reserve(dmnd_ctx* c, const SeedParams& sp, const SeedSizes& z, size_t bitmap_bytes, int64_t nq_pos, int64_t q_end, int64_t q_block_len, bool generous)
{
	if (int rc = c->seed_bitmap.ensure(std::max(z.bm_total, bitmap_bytes))) return rc;
	{
		const size_t held = c->qid_of.cap;
		if (int rc = c->qid_of.ensure((size_t)q_end * sizeof(uint32_t))) return rc;
		if (c->qid_of.cap != held) c->qid_of_version = ~(uint64_t)0;    // grown: the ids went with the old buffer (the new one may have its address)
	}
	if (int rc = c->mask_time.ensure((size_t)q_block_len + 256)) return rc;
	if (int rc = c->seed_keys.ensure((size_t)z.SB * (z.slots << z.slot_shift))) return rc;
	if (int rc = c->seed_need.ensure((size_t)(z.slots / 32 + SEED_NEED_FOLD_WORDS) * sizeof(uint32_t))) return rc;      // the map and, behind it, its folded copy (launch_seed_collect)
	if (int rc = c->seed_next.ensure((size_t)seed_build_work_words(nq_pos) * sizeof(uint32_t))) return rc;        // the build's work area (launch_seed_build)
	if (int rc = c->seed_qlist.ensure((size_t)z.SB * nq_pos * sizeof(uint32_t))) return rc;
	if (int rc = c->seed_qkeys.ensure((size_t)nq_pos * sizeof(uint32_t))) return rc;
	// (c->counters is shared with the masking calls that may run beside a reservation: the search allocates it itself)
	if (!generous) return DMND_OK;
	const int64_t m_cap = std::max<int64_t>((int64_t)1 << 22, 4 * nq_pos);
	if (int rc = c->matched_slot.ensure((size_t)m_cap * sizeof(uint32_t))) return rc;
	if (int rc = c->matched_loc.ensure((size_t)m_cap * sizeof(int64_t))) return rc;
	if (int rc = c->seed_hits.ensure(((size_t)1 << 20) * sizeof(dmnd_seed_hit))) return rc;
	if (int rc = c->seed_deferred.ensure(((size_t)1 << 18) * sizeof(SeedDeferred))) return rc;
	if (z.fused) {
		if (int rc = c->seed_survivors.ensure(((size_t)1 << 20) * sizeof(SeedSurvivor))) return rc;
		if (int rc = c->seed_qfold.ensure((size_t)(q_block_len + 1) / 2 + 64)) return rc;
	}
	else {
		// chain mode: the survivor and scored lists at the capacity its first search starts from
		if (int rc = c->seed_survivors.ensure(((size_t)1 << 20) * sizeof(SeedSurvivor))) return rc;
		if (int rc = c->seed_scored.ensure(((size_t)1 << 20) * sizeof(SeedScored))) return rc;
	}
	return DMND_OK;
}

int dmnd_seed_query_ids(dmnd_ctx* c)
{
	const std::vector<int64_t>& ql = c->limits[DMND_QUERY];
	if (ql.size() < 2) return DMND_OK;
	const size_t bytes = (size_t)ql.back() * sizeof(uint32_t);
	if (c->qid_of_version == c->query_limits_version && c->qid_of.cap >= bytes) return DMND_OK;
	if (int rc = c->qid_of.ensure(bytes)) return rc;
	HIP_TRY(launch_seed_qid(c->d_limits[DMND_QUERY].as<int64_t>(), (int64_t)ql.size() - 1, c->qid_of.as<uint32_t>(), c->stream));
	c->qid_of_version = c->query_limits_version;
	return DMND_OK;
}

extern "C" int dmnd_seed_reserve(dmnd_ctx* c, const dmnd_seed_params* params, int64_t query_block_len)
{
	if (!c || !params || query_block_len <= 512) return fail(DMND_E_ARG, "dmnd_seed_reserve: bad argument");
	SeedParams sp;
	std::memcpy(&sp, params, sizeof(sp));
	if (sp.n_shapes < 1 || sp.n_shapes > SEED_MAX_SHAPES) return fail(DMND_E_ARG, "dmnd_seed_reserve: unsupported seed configuration");
	HIP_TRY(hipSetDevice(c->device));
	const int64_t nq_pos = query_block_len - 512;             // a SequenceSet block: 256 padding letters on either side
	const SeedSizes z = seed_sizes(c, sp, nq_pos);
	// (the per-call hooks of a search are not a reservation's: the search itself ensures what they ask for)
	return seed_reserve(c, sp, z, seed_sizes_sliced(c, sp, nq_pos, z, SEED_SLICE_MAX_WORDS, 0).bm_total, nq_pos, query_block_len - 256, query_block_len, true);
}

namespace {

// The per-call hooks of a search: diagnostics, the tests' switches that force a path, and the capacities and sizes that stand in for
// the computed or the tuning value. Read per call (the tests set them per search) in ONE place, seed_hooks(): the driver names no
// other environment variable but the process-static DMND_SEED_PHASES. (DMND_SEED_FUSED and the test for DMND_SEED_MATCHED_CAP in
// seed_sizes stay there: dmnd_seed_reserve needs them too.)
struct SeedHooks {
	bool trace;                       // DMND_TRACE: host wall time of the call's parts (the kernel times do not show allocations, copies and waits), the summary lines
	int chain, tiled, slices;         // DMND_SEED_CHAIN, _TILED, _SLICES: -1 unset, 0 / 1 forces never / always
	int classes_long;                 // DMND_SEED_CLASSES_LONG: below 0 unset, 0 / not 0 forces off / on
	uint64_t slices_budget;           // DMND_SEED_SLICES_BUDGET_MB, in bytes, and ...
	int64_t slices_min_letters;       // ... DMND_SEED_SLICES_MIN_LETTERS stand in for the tuning values
	uint32_t slice_words;             // DMND_SEED_SLICE_WORDS: most words of a slice (tests: many slices of a small filter)
	bool slices_alloc_fail;           // DMND_SEED_SLICES_ALLOC_FAIL: the reference cache's allocations count as failed (tests: the fallback to the plain stream)
	uint64_t slices_filter_words;     // DMND_SEED_SLICES_FILTER_WORDS: words of the level-1 filter a sliced search builds (tests on small blocks, size sweeps; 0: seed_slices_filter_words' rule)
	int64_t matched_cap, survivor_cap, hit_cap, deferred_cap;      // DMND_SEED_MATCHED_CAP, _SURVIVOR_CAP, _HIT_CAP, _DEFERRED_CAP force the overflow / retry paths: the capacity a buffer starts from, instead of the one computed (0: unset; cap_or)
	int64_t sort_cap, readback_bytes; // the chain's two sizes: the tuning values (csrc/tuning.h), or what DMND_SEED_SORT_CAP / DMND_SEED_READBACK_BYTES say
};
SeedHooks seed_hooks()
{
	auto num = [](const char* name, long long unset) { const char* e = getenv(name); return e ? atoll(e) : unset; };
	auto forced = [](const char* name) { const char* e = getenv(name); return e ? (atoi(e) != 0 ? 1 : 0) : -1; };
	auto cap = [](const char* name) { const char* e = getenv(name); return e ? std::max<int64_t>(1, atoll(e)) : (int64_t)0; };
	SeedHooks h;
	h.trace = getenv("DMND_TRACE") != nullptr;
	h.chain = forced("DMND_SEED_CHAIN"); h.tiled = forced("DMND_SEED_TILED"); h.slices = forced("DMND_SEED_SLICES");
	{ const char* e = getenv("DMND_SEED_CLASSES_LONG"); h.classes_long = e ? atoi(e) : -1; }
	h.slices_budget = (uint64_t)std::max<long long>(0, num("DMND_SEED_SLICES_BUDGET_MB", tuning().seed_slices_budget_mb)) << 20;
	h.slices_min_letters = num("DMND_SEED_SLICES_MIN_LETTERS", tuning().seed_slices_min_letters);
	h.slice_words = (uint32_t)std::min<long long>(SEED_SLICE_MAX_WORDS, std::max<long long>(64, num("DMND_SEED_SLICE_WORDS", SEED_SLICE_MAX_WORDS)));
	h.slices_alloc_fail = forced("DMND_SEED_SLICES_ALLOC_FAIL") == 1;
	h.slices_filter_words = (uint64_t)std::max<long long>(0, num("DMND_SEED_SLICES_FILTER_WORDS", 0));
	h.matched_cap = cap("DMND_SEED_MATCHED_CAP"); h.survivor_cap = cap("DMND_SEED_SURVIVOR_CAP");
	h.hit_cap = cap("DMND_SEED_HIT_CAP"); h.deferred_cap = cap("DMND_SEED_DEFERRED_CAP");
	const int64_t sort_cap = cap("DMND_SEED_SORT_CAP");
	h.sort_cap = std::min<int64_t>(sort_cap ? sort_cap : tuning().seed_sort_cap, (int64_t)1 << 24);
	h.readback_bytes = std::min<int64_t>(std::max<int64_t>(0, num("DMND_SEED_READBACK_BYTES", tuning().seed_readback_bytes)), (int64_t)1 << 30);
	return h;
}
int64_t cap_or(int64_t hook, int64_t computed) { return hook ? hook : computed; }

// What a pipeline keeps of the counter block from shape to shape
struct PostState {
	unsigned long long hits_seen = 0;     // the hit counter as last read with a shape's deferred count ...
	bool hits_fresh = false;              // ... fresh: nothing appended since
	unsigned long long def_max = 0;       // most deferred pairs of a shape. Over the capacity of the list: that shape's deferred pass did not run
};
// the hit list of the fused pipeline: every survivor gives at most one hit
struct FusedHits { int64_t cap = 0, bound = 0; };

// One search: what is fixed once it is set up (check_blocks, geometry, ref_decide, ref_cache), its running state, and its phases in their order
struct SeedRun {
	dmnd_ctx* c;
	SeedHooks hooks;
	SeedParams sp;
	hipStream_t st;
	int64_t q_begin = 0, q_end = 0, t_begin = 0, t_end = 0, nq_pos = 0, n_targets = 0;
	int S = 0;
	SeedSizes z, z_sliced;            // the geometry in use; what it is (or would be) on the sliced stream (seed_sizes_sliced) -- z from ref_decide on
	int slot_bits = 0, bm_log2 = 0;   // log2(slots): the sort key of the build (SeedArgs::order) and of the tiled filter's sort; log2 of the level-2 filter's words
	size_t slot_bytes = 0;            // one shape's table
	bool nibble_shapes = true, classes_long = false;
	int classes = 0;
	bool mlr_on = false, lin_on = false, phases = false;      // mutual coverage, linearised search, DMND_SEED_PHASES
	bool index_ready = false;         // the query side is kept from the last call (query index reuse, under this signature)
	std::string signature;
	int64_t tiled_from = 0;           // joined positions of a shape from which on its pair filter is the tiled one
	SeedRefUse ref_use = SEED_REF_NONE;      // the sliced stream
	int slice_bits = -1;
	int64_t ref_windows = 0;
	std::vector<unsigned long long> counts;  // joined positions per shape ...
	std::vector<int64_t> m_off;              // ... and where a shape's begin in the lists that the shapes share (phases 1 and 2)
	bool pristine = true;             // the counters and the need map are as the first clear left them
	Timer tm;
	char path[128] = "host";          // DMND_TRACE: the path the search took (seed_chain.h)
	unsigned long long n_pairs = 0;
	std::chrono::steady_clock::time_point lap_t0 = std::chrono::steady_clock::now();

	SeedRun(dmnd_ctx* ctx, const SeedHooks& h) : c(ctx), hooks(h), st(ctx->stream), tm(ctx->stream) {}
	int check_blocks();
	int geometry();
	void ref_decide();
	int prepare();
	int ref_cache();
	int fused();
	int fused_stage2(SeedArgs a, int sid, unsigned long long n, unsigned long long ns, FusedHits& fh, PostState& ps);
	int after_post(const SeedArgs& a, int sid, int64_t n_matched, int64_t def_cap, PostState& ps);
	SeedArgs chain_args(const SeedChain& ch, int64_t def_cap, int sid) const;
	int chain(ChainResume& res);
	int phase1(const ChainResume& res);
	int count_pairs();
	int phase2(const ChainResume& res);
	int pair_filter(SeedArgs& a, int sid);
	int sort_hits();
	void trace_summary() const;

	void lap(const char* what) const
	{
		if (hooks.trace) std::fprintf(stderr, "dmnd_seed_search %8.2f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - lap_t0).count(), what);
	}
	unsigned long long* ctr() const { return c->counters.as<unsigned long long>(); }

	// the kernels' arguments of shape sid, its joined positions in the matched_cap entries from matched_off of the shared lists
	SeedArgs args_for(int sid, int64_t matched_cap, int64_t matched_off) const
	{
		const int own = sid % z.SB;                        // which of the SB buffer sets the shape uses
		SeedArgs a;
		a.params = sp;
		a.qdata = c->block[DMND_QUERY].as<int8_t>(); a.tdata = c->block[DMND_TARGET].as<int8_t>();
		// motif soft masking: seeds come from the masked views; the query-indexed algorithm does not soft-mask the reference
		// block (search/stage0.cpp:125-127)
		a.qseed = c->soft_valid[DMND_QUERY] ? c->soft[DMND_QUERY].as<int8_t>() : a.qdata;
		a.tseed = (c->soft_valid[DMND_TARGET] && sp.seed_encoding == SEED_SPACED) ? c->soft[DMND_TARGET].as<int8_t>() : a.tdata;
		a.qlimits = c->d_limits[DMND_QUERY].as<int64_t>();
		a.q_begin = q_begin; a.q_end = q_end; a.t_begin = t_begin; a.t_end = t_end;
		a.qid_of = c->qid_of.as<uint32_t>(); a.mask_time = c->mask_time.as<uint8_t>();
		a.tlimits = c->d_limits[DMND_TARGET].as<int64_t>(); a.n_targets = n_targets;
		a.qwin = mlr_on ? c->seed_qwin.as<SeedQueryWindow>() : nullptr;
		a.lin_first = lin_on ? c->seed_lin_first.as<int64_t>() : nullptr;
		a.slots = reinterpret_cast<SeedSlot*>(c->seed_keys.as<char>() + (size_t)own * slot_bytes);
		a.slot_shift = z.slot_shift;
		a.qlist = c->seed_qlist.as<uint32_t>() + (size_t)own * nq_pos;
		a.slot_mask = z.slots - 1;
		a.classes = classes;
		a.slot_bits = slot_bits;
		a.bm1_hmask = bm1_hmask_of(slot_bits, classes);
		a.bitmap_log2 = bm_log2;
		a.phase_ticks = phases ? ctr() + S + 8 : nullptr;
		a.tclass = classes ? c->seed_tclass.as<uint16_t>() : nullptr; a.tclass_stride = (seed_code_groups(t_begin, t_end) + 3) & ~(int64_t)3;
		a.tcodes = classes ? c->seed_tcodes.as<uint64_t>() : nullptr; a.tflags = classes ? c->seed_tflags.as<uint32_t>() : nullptr; a.tplanes = classes ? c->seed_tplanes.as<uint64_t>() : nullptr;
		a.bitmap = c->seed_bitmap.as<uint32_t>() + (size_t)own * (z.bm_words + z.bm1_words);
		a.bitmap1 = a.bitmap + z.bm_words;
		a.bitmap1_words = (uint32_t)z.bm1_words; a.bitmap1_k3 = z.bm1_k3;
		a.matched_slot = c->matched_slot.as<uint32_t>() + matched_off;
		a.matched_loc = c->matched_loc.as<int64_t>() + matched_off;
		a.matched_count = ctr() + sid;
		a.matched_cap = matched_cap;
		a.deferred = nullptr; a.deferred_count = ctr() + S + 1; a.deferred_cap = 0;
		a.survivors = nullptr; a.survivor_count = ctr() + S + 3; a.survivor_cap = 0;
		a.scored = nullptr; a.scored_count = ctr() + S + 4;
		a.need_bits = c->seed_need.as<uint32_t>();
		a.e_key = nullptr; a.e_count = ctr() + S + 2; a.e_n = 0;
		a.matrix = c->matrix.as<int8_t>();
		a.hits = c->seed_hits.as<dmnd_seed_hit>(); a.hit_count = ctr() + S; a.hit_cap = 0;
		a.fused = z.fused ? 1 : 0;
		a.level2 = sp.shape_weight[sid] >= 10 ? 1 : 0;
		a.qfold = z.fused ? c->seed_qfold.as<uint8_t>() : nullptr;
		a.tfold = z.fused ? c->seed_tfold.as<uint8_t>() : nullptr;
		return a;
	}

	// ... for phase 2 (and the chain, which runs it on the device): with the hit and deferred lists where they are now
	SeedArgs args_with_lists(int sid, int64_t matched_cap, int64_t matched_off, int64_t hit_cap, int64_t def_cap) const
	{
		SeedArgs a = args_for(sid, matched_cap, matched_off);
		a.hits = c->seed_hits.as<dmnd_seed_hit>(); a.hit_cap = hit_cap;
		a.deferred = c->seed_deferred.as<SeedDeferred>(); a.deferred_cap = def_cap;
		return a;
	}

	// the stream of one shape: the sliced kernel over the cache, or the plain one
	hipError_t stream_shape(const SeedArgs& a, int sid) const
	{
		if (ref_use == SEED_REF_NONE) return launch_seed_stream(a, sid, st);
		return launch_seed_stream_slices(a, sid, c->seed_ref_codes.as<uint64_t>(), c->seed_ref_lists.as<uint32_t>() + (size_t)sid * (size_t)ref_windows,
			c->seed_ref_hashes.as<uint32_t>() + (size_t)sid * (size_t)ref_windows, c->seed_ref_counts.as<uint32_t>() + (size_t)sid * 64, slice_bits, st);
	}

	// the query side of one shape: built (table, position lists, bitmaps), or -- kept from an earlier call -- its marks reset
	int query_side(const SeedArgs& a, int sid, bool build) const
	{
		if (build) {
			HIP_TRY(launch_seed_build(a, sid, c->seed_qlist.as<uint32_t>() + (size_t)(sid % z.SB) * nq_pos, c->seed_next.as<uint32_t>(), c->seed_qkeys.as<uint32_t>(),
				&c->sort_tmp, &c->sort_tmp_bytes, st));
		}
		else HIP_TRY(launch_seed_reset(a, sid, st));
		return DMND_OK;
	}
};

int seed_check_params(const SeedParams& sp)
{
	if (sp.n_shapes < 1 || sp.n_shapes > SEED_MAX_SHAPES || sp.index_chunks < 1 || sp.seedp_bits < 1 || sp.seedp_bits > 24
		|| sp.n_shapes * sp.index_chunks >= SEED_NEVER || sp.ungapped_window < 1 || sp.ungapped_window > 128 || sp.reduction_size < 2)
		return fail(DMND_E_ARG, "dmnd_seed_search: unsupported seed configuration");
	// seed_is_complex counts reduced letters in count[20] and indexes LNFACT[20] by the counts (<= weight): weight <= 19, classes <= 20
	if (sp.reduction_size > 20) return fail(DMND_E_ARG, "dmnd_seed_search: more than 20 reduced letter classes");
	for (int l = 0; l < 32; ++l)
		if (!((sp.reduction[l] >= 0 && sp.reduction[l] < sp.reduction_size) || sp.reduction[l] == L_MASK))
			return fail(DMND_E_ARG, "dmnd_seed_search: reduction map entry outside [0, reduction_size) and not the mask letter");
	for (int i = 0; i < sp.n_shapes; ++i) {
		if (sp.shape_len[i] < 1 || sp.shape_len[i] > 32 || sp.shape_weight[i] < 1 || sp.shape_weight[i] > 19 || sp.shape_weight[i] > sp.shape_len[i])
			return fail(DMND_E_ARG, "dmnd_seed_search: bad shape (length 1..32, weight 1..19)");
		uint32_t mask = 0;
		for (int k = 0; k < sp.shape_weight[i]; ++k) {
			if (sp.shape_pos[i][k] < 0 || sp.shape_pos[i][k] >= sp.shape_len[i]) return fail(DMND_E_ARG, "dmnd_seed_search: shape position outside the shape");
			mask |= 1u << sp.shape_pos[i][k];
		}
		if (mask != sp.shape_mask[i]) return fail(DMND_E_ARG, "dmnd_seed_search: shape mask and positions disagree");
	}
	if (sp.seed_encoding != SEED_SPACED && sp.seed_encoding != SEED_HASHED) return fail(DMND_E_ARG, "dmnd_seed_search: unknown seed encoding");
	if (sp.seed_encoding == SEED_HASHED) {
		if (sp.index_chunks != 1 || sp.reduction_size > 16) return fail(DMND_E_ARG, "dmnd_seed_search: the query-indexed mode runs with one index chunk and a 4-bit reduction");
		for (int i = 0; i < sp.n_shapes; ++i)
			if (sp.shape_len[i] > 16) return fail(DMND_E_ARG, "dmnd_seed_search: query-indexed mode with a shape longer than 16 letters");
	}
	return DMND_OK;
}

// what the mutual-coverage and the linearised search want of the blocks
int SeedRun::check_blocks()
{
	const std::vector<int64_t>& ql = c->limits[DMND_QUERY];
	const std::vector<int64_t>& tl = c->limits[DMND_TARGET];
	// mutual-coverage search (length_ratio_core.h): the windows of the pair filters are ranges only over length-sorted blocks
	mlr_on = c->min_length_ratio > 0.0;
	c->seed_qwin_n = 0;
	if (mlr_on) {
		if (c->query_contexts != 1 || sp.query_translated) return fail(DMND_E_ARG, "dmnd_seed_search: a minimum length ratio is not supported for translated searches");
		if (!lengths_non_increasing(ql.data(), (int64_t)ql.size() - 1)) return fail(DMND_E_ARG, "dmnd_seed_search: with a minimum length ratio the query block must be length-sorted (dmnd_length_sort_order)");
		if (!lengths_non_increasing(tl.data(), (int64_t)tl.size() - 1)) return fail(DMND_E_ARG, "dmnd_seed_search: with a minimum length ratio the reference block must be length-sorted (dmnd_length_sort_order)");
	}
	// linearised search (linsearch_core.h): the first position of a seed lies in its longest target only over a length-sorted reference block
	lin_on = c->linsearch;
	if (lin_on) {
		for (int i = 0; i < sp.n_shapes; ++i)
			if (!lin_shape_weight_ok(sp.shape_weight[i])) return fail(DMND_E_ARG, "dmnd_seed_search: Linearization is only supported for seed shapes of weight >= 10.");
		if (mlr_on) return fail(DMND_E_ARG, "dmnd_seed_search: the linearised search together with a minimum length ratio is not supported (dmnd_set_linsearch, dmnd_set_min_length_ratio)");
		if (c->lin_sorted_generation != c->target_generation) {
			if (!lengths_non_increasing(tl.data(), (int64_t)tl.size() - 1)) return fail(DMND_E_ARG, "dmnd_seed_search: the linearised search wants the reference block length-sorted (dmnd_length_sort_order)");
			c->lin_sorted_generation = c->target_generation;
		}
	}
	return DMND_OK;
}

// buffer geometry, key classes, the signature of a kept query index
int SeedRun::geometry()
{
	if (nq_pos >= 0xffffffffLL) return fail(DMND_E_ARG, "dmnd_seed_search: query block larger than 4G letters");
	S = sp.n_shapes;
	z = seed_sizes(c, sp, nq_pos);
	z_sliced = seed_sizes_sliced(c, sp, nq_pos, z, hooks.slice_words, hooks.slices_filter_words);
	if (z.slots > ((uint64_t)1 << 31)) return fail(DMND_E_ARG, "dmnd_seed_search: query block too large for 32-bit slot numbers (more than 1.7 G seed positions): cut it into smaller blocks");
	slot_bytes = (size_t)z.slots << z.slot_shift;
	while (((uint64_t)1 << slot_bits) < z.slots) ++slot_bits;
	while (((uint64_t)1 << bm_log2) < z.bm_words) ++bm_log2;
	// key classes (seed_core.h seed_class): the short-seed pipeline, whose stream has no form without them ...
	// ... and (round 5) long seeds against a query block whose level-1 filter has outgrown an XCD's L2 (above 2^24 query positions the
	// filter is 4-16 MB: C5's 100 000 queries): by class every XCD probes its own eighth of it. DMND_SEED_CLASSES_LONG=0/1 forces it.
	for (int i = 0; i < S; ++i) nibble_shapes = nibble_shapes && seed_nibble_mode(sp, i);
	classes_long = !z.fused && nibble_shapes && (hooks.classes_long >= 0 ? hooks.classes_long != 0 : SEED_CLASSES_LONG_DEFAULT && z.bm1_words * 32 >= ((uint64_t)1 << 25));      // (C2's 3 MB filter stays on the plain stream: by class it took 2.57 ms against 1.46)
	classes = (z.fused || classes_long) && z.slots >= 64 && z.bm1_words % 8 == 0 && z.bm1_words >= 64 ? 8 : 0;
	// (seed_sizes gives every fused search at least 1024 slots and a level-1 filter of 2^k >= 2^15 words)
	if (z.fused && !classes) return fail(DMND_E_ARG, "dmnd_seed_search: fused seed search without key classes (table or level-1 filter too small for eighths)");
	if (z.reuse) {
		signature.assign(reinterpret_cast<const char*>(&sp), sizeof(sp));
		const uint64_t extra[7] = { c->query_generation, (uint64_t)nq_pos, z.slots, z.bm_words, z.bm1_words, (uint64_t)z.fused + 2 * (uint64_t)classes, (uint64_t)z.slot_shift * 4 + z.bm1_k3 };
		signature.append(reinterpret_cast<const char*>(extra), sizeof(extra));
	}
	index_ready = z.reuse && c->qindex_signature == signature && !signature.empty();
	c->qindex_signature.clear();                         // set again when this call has built (or kept) a complete index
	// many joined positions (short seeds): sorted by seed for the LDS-tiled pair filter; otherwise one thread per position. DMND_SEED_TILED=0/1 forces it
	tiled_from = hooks.tiled < 0 ? (int64_t)1 << 22 : hooks.tiled ? 0 : INT64_MAX;
	static const bool phases_on = getenv("DMND_SEED_PHASES") != nullptr;
	phases = phases_on;
	counts.assign((size_t)S + 1, 0); m_off.assign((size_t)S + 1, 0);
	lap("parameters checked");
	return DMND_OK;
}

// the buffers of the geometry, and everything a search starts from enqueued: the one clear, query windows, query ids, folds, codes
int SeedRun::prepare()
{
	if (int rc = seed_reserve(c, sp, z, z_sliced.bm_total, nq_pos, q_end, c->block_len[DMND_QUERY], false)) return rc;
	if (lin_on) {                                       // (never cleared: the reduction initialises the slots it reads, seed_lin_first_kernel)
		if (z.fused) return fail(DMND_E_ARG, "dmnd_seed_search: the linearised search has no form in the fused short-seed pipeline");
		if (int rc = c->seed_lin_first.ensure((size_t)z.slots * sizeof(int64_t))) return rc;
	}
	lap("buffers ensured");
	const bool counters_new = c->counters.cap < (size_t)chain_ctr_words(S) * sizeof(unsigned long long);
	if (int rc = c->counters.ensure((size_t)chain_ctr_words(S) * sizeof(unsigned long long))) return rc;      // [S] hits, [S+1] deferred pairs, [S+2] collected positions, [S+3] Hamming survivors, [S+4] scored survivors, [S+5 ..] chain mode (seed_chain.h)
	// everything a search starts from, in ONE launch (launch_seed_clear): the counters, the mask times, the need map and -- unless the
	// query side is kept from the last call -- bitmaps and table
	{
		SeedClear clr;
		clr.add(c->counters.p, (size_t)((phases || counters_new) ? S + 16 : S + 8) * sizeof(unsigned long long), 0);
		clr.add(c->mask_time.p, (size_t)c->block_len[DMND_QUERY] + 256, SEED_NEVER);
		clr.add(c->seed_need.p, (size_t)(z.slots / 32) * sizeof(uint32_t), 0);
		if (!index_ready) {
			clr.add(c->seed_bitmap.p, z.bm_total, 0);
			clr.add(c->seed_keys.p, (size_t)z.SB * slot_bytes, 0xff);
		}
		HIP_TRY(launch_seed_clear(clr, st));
	}
	if (mlr_on) {                                       // per target of THIS reference block: rebuilt by every call, whatever is kept of the query side
		if (int rc = c->seed_qwin.ensure((size_t)n_targets * sizeof(SeedQueryWindow))) return rc;
		HIP_TRY(launch_seed_qwin(c->d_limits[DMND_QUERY].as<int64_t>(), (int64_t)c->limits[DMND_QUERY].size() - 1, c->d_limits[DMND_TARGET].as<int64_t>(), n_targets, c->min_length_ratio, c->seed_qwin.as<SeedQueryWindow>(), st));
		c->seed_qwin_n = n_targets;
	}
	if (int rc = dmnd_seed_query_ids(c)) return rc;      // (filled at the upload: nothing to do here but for a shared block or a grown buffer)
	// fused pipeline: 4-bit copies of the query and the reference block for the Hamming pre-filter
	if (z.fused) {
		const int64_t nq = c->block_len[DMND_QUERY], nt = c->block_len[DMND_TARGET];
		if (int rc = c->seed_qfold.ensure((size_t)(nq + 1) / 2 + 64)) return rc;
		if (int rc = c->seed_tfold.ensure((size_t)(nt + 1) / 2 + 64)) return rc;
		HIP_TRY(launch_seed_fold(c->block[DMND_QUERY].as<int8_t>(), nq, c->seed_qfold.as<uint8_t>(), st));
		HIP_TRY(launch_seed_fold(c->block[DMND_TARGET].as<int8_t>(), nt, c->seed_tfold.as<uint8_t>(), st));
	}
	if (classes) {
		const int8_t* tseed = (c->soft_valid[DMND_TARGET] && sp.seed_encoding == SEED_SPACED) ? c->soft[DMND_TARGET].as<int8_t>() : c->block[DMND_TARGET].as<int8_t>();
		const int64_t n = seed_code_groups(t_begin, t_end);
		if (int rc = c->seed_tcodes.ensure((size_t)n * sizeof(uint64_t))) return rc;
		if (int rc = c->seed_tflags.ensure((size_t)n * sizeof(uint32_t))) return rc;
		if (int rc = c->seed_tplanes.ensure((size_t)n * sizeof(uint64_t))) return rc;
		if (int rc = c->seed_tclass.ensure((size_t)9 * (size_t)((n + 3) & ~(int64_t)3) * sizeof(uint16_t))) return rc;      // planes of a stride that is a multiple of four groups: 8-byte stores
		HIP_TRY(launch_seed_codes(sp, tseed, t_begin, t_end, c->seed_tcodes.as<uint64_t>(), c->seed_tflags.as<uint32_t>(), c->seed_tplanes.as<uint64_t>(), st));
	}
	for (int i = 0; i < 5; ++i) c->seed_ms[i] = 0;
	lap("clears and query ids enqueued");
	return DMND_OK;
}

// ---- Sliced long-seed stream (seed_slices_core.h): long spaced seeds on the plain path (not fused, no key classes,
// nibble shapes) probe the level-1 filter from LDS slices, over a routing of the reference windows that is kept per uploaded block.
// Hashed (query-indexed) seeds stay on the plain kernel: their windows with a mask / stop letter are keyed from the raw letters.
// The first search of a block generation takes the plain kernel and builds nothing (a block searched once pays nothing), the second
// one with the same key builds, later ones keep. DMND_SEED_SLICES=0/1 forces never / always (always: built by the first search),
// DMND_SEED_SLICES_BUDGET_MB and DMND_SEED_SLICES_MIN_LETTERS stand in for the tuning values (SeedHooks).
// ref_decide decides (ref_use, slice_bits, ref_windows) and with them the geometry, before anything is reserved or cleared for it:
// a search on the sliced stream takes z_sliced, whose level-1 filter is sized for LDS slices (C2: 64 x 128 KB instead of 3 MB),
// every other search seed_sizes' geometry. The cache's key holds the slice count of z_sliced whatever stream this search takes, so
// that the plain first search of a block and the sliced ones behind it agree on it. ref_cache builds the reference-side cache
// where the decision is to build.
void SeedRun::ref_decide()
{
	ref_windows = seed_ref_windows(t_begin, t_end);
	slice_bits = seed_slice_bits(z_sliced.bm1_words, slot_bits, hooks.slice_words);
	// The default rule takes the sliced stream where it was measured to win: a sparse level-1 filter -- at least four bits per query
	// position, C2's 3 % positives: what the slices save is the probe that ends at level 1; C4's filter (1e7
	// query seeds, a third of the probes positive) took 4.29 ms by slices against 3.52 -- and few joins in the context's last search
	// (the sliced stream lists the joins slice by slice, not in block order: C2skew).
	const bool sparse_filter = (uint64_t)nq_pos * 4 <= z.bm1_words * 32;      // (at least four filter bits per query position: seed_sizes' own bound for the third bit)
	const bool eligible = !z.fused && !classes && nibble_shapes && sp.seed_encoding == SEED_SPACED && slice_bits >= 0 && ref_windows < ((int64_t)1 << 31)
		&& (hooks.slices == 1 || (t_end - t_begin >= hooks.slices_min_letters && sparse_filter && c->seed_last_joined <= tuning().seed_slices_max_joined));
	const int8_t* tseed = c->soft_valid[DMND_TARGET] ? c->soft[DMND_TARGET].as<int8_t>() : c->block[DMND_TARGET].as<int8_t>();
	bool drop = false;
	ref_use = seed_ref_decide(c->seed_ref, seed_ref_key_of(c->target_generation, tseed, t_begin, t_end, sp, slice_bits), hooks.slices, eligible, seed_ref_cache_bytes(t_begin, t_end, S) + seed_ref_hash_bytes(t_begin, t_end, S), hooks.slices_budget, &drop);
	if (drop) c->release_seed_ref_buffers();            // (nothing on the stream reads them: the last search has been waited for; the state is seed_ref_decide's)
	if (ref_use != SEED_REF_NONE) z = z_sliced;
}

int SeedRun::ref_cache()
{
	if (ref_use != SEED_REF_BUILT) return DMND_OK;
	const int8_t* tseed = c->soft_valid[DMND_TARGET] ? c->soft[DMND_TARGET].as<int8_t>() : c->block[DMND_TARGET].as<int8_t>();
	// class nibbles (kept), flags and routing bytes (scratch of the build), then per shape one radix pass into its lists.
	// An allocation that fails leaves the search on the plain kernel.
	const int64_t n_groups = seed_code_groups(t_begin, t_end);
	DevBuf route[2];
	// (the kept buffers at their exact size, not with the slack DevBuf::ensure adds for buffers that grow: the budget counts these bytes)
	auto exact = [](DevBuf& b, size_t bytes) {
		if (b.cap == bytes && b.own) return true;
		b.release();
		if (hipMalloc(&b.p, bytes) != hipSuccess) { b.p = nullptr; (void)hipGetLastError(); return false; }
		b.cap = bytes;
		return true;
	};
	const bool ok = !hooks.slices_alloc_fail && exact(c->seed_ref_codes, (size_t)n_groups * sizeof(uint64_t)) && c->seed_tflags.ensure((size_t)n_groups * sizeof(uint32_t)) == DMND_OK
		&& exact(c->seed_ref_lists, (size_t)S * (size_t)ref_windows * sizeof(uint32_t)) && exact(c->seed_ref_hashes, (size_t)S * (size_t)ref_windows * sizeof(uint32_t))
		&& exact(c->seed_ref_counts, (size_t)S * 64 * sizeof(uint32_t))
		&& exact(route[0], (size_t)ref_windows) && exact(route[1], (size_t)ref_windows);
	if (ok) {
		tm.start();
		hipError_t e = launch_seed_codes(sp, tseed, t_begin, t_end, c->seed_ref_codes.as<uint64_t>(), c->seed_tflags.as<uint32_t>(), nullptr, st);
		for (int sid = 0; sid < S && e == hipSuccess; ++sid) {
			uint32_t* list = c->seed_ref_lists.as<uint32_t>() + (size_t)sid * (size_t)ref_windows;
			e = launch_seed_route(sp, sid, c->seed_ref_codes.as<uint64_t>(), c->seed_tflags.as<uint32_t>(), t_begin, t_end, slice_bits, route[0].as<uint8_t>(), route[1].as<uint8_t>(),
				list, c->seed_ref_counts.as<uint32_t>() + (size_t)sid * 64, &c->sort_tmp, &c->sort_tmp_bytes, st);
			if (e == hipSuccess) e = launch_seed_ref_hashes(sp, sid, c->seed_ref_codes.as<uint64_t>(), list, t_begin, t_end, c->seed_ref_hashes.as<uint32_t>() + (size_t)sid * (size_t)ref_windows, st);
		}
		tm.stop(c->seed_ms[0]);
		if (e == hipSuccess) e = sync_stream(st);          // the scratch goes away below
		if (e != hipSuccess) { route[0].release(); route[1].release(); c->release_seed_ref(); HIP_TRY(e); }
	}
	route[0].release(); route[1].release();
	seed_ref_built(c->seed_ref, ok);
	if (!ok) {
		// the plain stream after all, with its own geometry: the query side is not built yet. Where the geometry differs, the filters
		// (reserved for either one) are cleared again where this one has them; where it is the same -- always with a kept query
		// index, whose filters prepare() left as they are -- nothing is touched
		c->release_seed_ref(); ref_use = SEED_REF_NONE;
		const SeedSizes plain = seed_sizes(c, sp, nq_pos);
		const bool moved = plain.bm1_words != z.bm1_words || plain.bm1_k3 != z.bm1_k3;
		z = plain;
		if (moved && !index_ready) {
			SeedClear clr;
			clr.add(c->seed_bitmap.p, z.bm_total, 0);
			HIP_TRY(launch_seed_clear(clr, st));
		}
	}
	lap("reference cache built");
	return DMND_OK;
}

// Pairs scoring above 255 (rare): the second pass that resolves the reference's SIMD-batch saturation rule for the nd deferred
// pairs of shape sid. The joined positions of the seeds that own one (of the n_matched in a.matched_*) are collected, sorted by
// (slot, position), and scored again.
int seed_deferred_pass(dmnd_ctx* c, SeedArgs a, int sid, int64_t n_matched, int64_t nd, hipStream_t st)
{
	if (int rc = c->seed_eslot.ensure((size_t)n_matched * sizeof(uint64_t))) return rc;      // unsorted keys
	if (int rc = c->seed_eloc.ensure((size_t)n_matched * sizeof(uint64_t))) return rc;       // sorted keys
	a.e_key = c->seed_eslot.as<uint64_t>();
	HIP_TRY(launch_seed_collect(a, n_matched, st));
	unsigned long long ne = 0;
	HIP_TRY(copy_now(st, &ne, a.e_count, sizeof(ne), hipMemcpyDeviceToHost));
	HIP_TRY(sort_keys_u64(c->seed_eslot.as<uint64_t>(), c->seed_eloc.as<uint64_t>(), (int64_t)ne, &c->sort_tmp, &c->sort_tmp_bytes, st));
	a.e_key = c->seed_eloc.as<uint64_t>();
	a.e_n = (int64_t)ne;
	HIP_TRY(launch_seed_deferred(a, sid, nd, st));
	return DMND_OK;
}

// Behind a shape's post kernels (launch_seed_post), where the ungapped filter is on: pairs scoring above 255 (rare) go through the
// second pass. (hits so far, deferred pairs of this shape) are neighbours in the counter block: one copy -- and with nothing deferred
// behind the search's last shape that hit count is already the final one. More deferred pairs than def_cap: the list is incomplete,
// no pass (the caller sees ps.def_max).
int SeedRun::after_post(const SeedArgs& a, int sid, int64_t n_matched, int64_t def_cap, PostState& ps)
{
	ps.hits_fresh = false;
	if (!sp.use_ungapped) return DMND_OK;
	unsigned long long both[2] = { 0, 0 };
	HIP_TRY(copy_now(st, both, a.hit_count, sizeof(both), hipMemcpyDeviceToHost));
	const unsigned long long nd = both[1];
	c->seed_trace[S + sid] = nd;
	if (nd == 0) { ps.hits_seen = both[0]; ps.hits_fresh = true; return DMND_OK; }
	ps.def_max = std::max(ps.def_max, nd);
	if ((int64_t)nd > def_cap) return DMND_OK;
	tm.start();
	if (int rc = seed_deferred_pass(c, a, sid, n_matched, (int64_t)nd, st)) return rc;
	tm.stop(c->seed_ms[3]);
	return DMND_OK;
}

// ---- stage 2 of the fused pipeline: everything behind a shape's Hamming filter (stage-2 scores, left-most rule, deferred pairs) for
// its n joined positions and ns survivors, on the same stream
int SeedRun::fused_stage2(SeedArgs a, int sid, unsigned long long n, unsigned long long ns, FusedHits& fh, PostState& ps)
{
	if (fh.bound + (int64_t)ns > fh.cap) {               // grow, keeping the hits of the earlier shapes
		const int64_t new_cap = fh.bound + (int64_t)ns + (fh.bound + (int64_t)ns) / 2;
		DevBuf nb;
		if (int rc = nb.ensure((size_t)new_cap * sizeof(dmnd_seed_hit))) return rc;
		HIP_TRY(hipMemcpyAsync(nb.p, c->seed_hits.p, (size_t)fh.cap * sizeof(dmnd_seed_hit), hipMemcpyDeviceToDevice, st));
		HIP_TRY(sync_stream(st));
		c->seed_hits.release();
		c->seed_hits = nb;
		fh.cap = new_cap;
	}
	fh.bound += (int64_t)ns;
	if (int rc = c->seed_deferred.ensure((size_t)ns * sizeof(SeedDeferred))) return rc;      // deferred pairs <= survivors
	a.hits = c->seed_hits.as<dmnd_seed_hit>(); a.hit_cap = fh.cap;
	a.deferred = c->seed_deferred.as<SeedDeferred>(); a.deferred_cap = (int64_t)ns;
	if (int rc = c->seed_scored.ensure((size_t)ns * sizeof(SeedScored))) return rc;
	a.scored = c->seed_scored.as<SeedScored>();
	tm.start();
	{
		// this stage's own counters (deferred pairs, collected positions, scored) and the need map
		SeedClear clr;
		clr.add(ctr() + S + 1, 2 * sizeof(unsigned long long), 0);
		clr.add(ctr() + S + 4, sizeof(unsigned long long), 0);
		clr.add(c->seed_need.p, (size_t)(z.slots / 32) * sizeof(uint32_t), 0);
		HIP_TRY(launch_seed_clear(clr, st));
	}
	HIP_TRY(launch_seed_post(a, sid, (int64_t)ns, st, false));
	tm.stop(c->seed_ms[3]);
	return after_post(a, sid, (int64_t)n, (int64_t)ns, ps);      // (a deferred list as long as the survivor list never overflows)
}

// Short seeds: one pass per shape -- index, stream with the Hamming filter fused in, mask, stage-2 scoring of the survivors,
// deferred pairs. A shape's masks only depend on this and earlier shapes, and so does the left-most rule (t_now).
int SeedRun::fused()
{
	const int SB = z.SB;
	int64_t m_cap = cap_or(hooks.matched_cap, std::max<int64_t>(std::max<int64_t>((int64_t)1 << 22, 4 * nq_pos), (int64_t)(std::min(c->matched_loc.cap / sizeof(int64_t), c->matched_slot.cap / sizeof(uint32_t)))));
	int64_t surv_cap = cap_or(hooks.survivor_cap, std::max<int64_t>((int64_t)1 << 20, (int64_t)(c->seed_survivors.cap / sizeof(SeedSurvivor))));
	FusedHits fh;
	fh.cap = cap_or(hooks.hit_cap, std::max<int64_t>((int64_t)1 << 20, (int64_t)(c->seed_hits.cap / sizeof(dmnd_seed_hit))));
	if (int rc = c->seed_hits.ensure((size_t)fh.cap * sizeof(dmnd_seed_hit))) return rc;
	c->seed_trace.assign((size_t)2 * S, 0);
	std::vector<unsigned long long> host_ctr((size_t)S + 4);
	PostState ps;
	const bool recycle = SB < S;                          // a buffer set serves several shapes: cleared before its next one
	for (int sid = 0; sid < S; ++sid) {
		SeedArgs a = args_for(sid, 0, 0);
		tm.start();
		if (sid > 0) {
			// the survivor counter and, where a buffer set is used again, its table and bitmaps -- one launch
			SeedClear clr;
			clr.add(ctr() + S + 3, sizeof(unsigned long long), 0);
			if (recycle && sid >= SB) {
				const size_t own = (size_t)(sid % SB);
				clr.add(c->seed_keys.as<char>() + own * slot_bytes, slot_bytes, 0xff);
				clr.add(c->seed_bitmap.as<char>() + own * (size_t)(z.bm_words + z.bm1_words) * sizeof(uint32_t), (size_t)(z.bm_words + z.bm1_words) * sizeof(uint32_t), 0);
			}
			HIP_TRY(launch_seed_clear(clr, st));
		}
		if (int rc = query_side(a, sid, !index_ready)) return rc;
		tm.stop(c->seed_ms[0]);
		unsigned long long n = 0, ns = 0;
		for (int attempt = 0;; ++attempt) {
			if (int rc = c->matched_slot.ensure((size_t)m_cap * sizeof(uint32_t))) return rc;
			if (int rc = c->matched_loc.ensure((size_t)m_cap * sizeof(int64_t))) return rc;
			if (int rc = c->seed_survivors.ensure((size_t)surv_cap * sizeof(SeedSurvivor))) return rc;
			a.matched_slot = c->matched_slot.as<uint32_t>(); a.matched_loc = c->matched_loc.as<int64_t>(); a.matched_cap = m_cap;
			a.survivors = c->seed_survivors.as<SeedSurvivor>(); a.survivor_cap = surv_cap;
			if (attempt > 0) {                               // (the first attempt finds them zero: the clears above)
				HIP_TRY(hipMemsetAsync(a.matched_count, 0, sizeof(unsigned long long), st));
				HIP_TRY(hipMemsetAsync(a.survivor_count, 0, sizeof(unsigned long long), st));
			}
			tm.start();
			HIP_TRY(launch_seed_stream(a, sid, st, true));
			tm.stop(c->seed_ms[1]);
			HIP_TRY(copy_now(st, host_ctr.data(), ctr(), host_ctr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
			n = host_ctr[sid]; ns = host_ctr[S + 3];
			if ((int64_t)n <= m_cap && (int64_t)ns <= surv_cap) break;
			if (attempt >= 2) return fail(DMND_E_NOMEM, "dmnd_seed_search: joined-position / survivor buffer overflow");
			if ((int64_t)n > m_cap) m_cap = (int64_t)n + (int64_t)n / 8 + 1024;
			if ((int64_t)ns > surv_cap) surv_cap = (int64_t)ns + (int64_t)ns / 8 + 1024;
		}
		counts[sid] = n;
		c->seed_trace[sid] = ns;
		if (sp.seed_encoding == SEED_SPACED) {
			tm.start();
			HIP_TRY(launch_seed_mask(a, sid, st));
			tm.stop(c->seed_ms[2]);
		}
		if (ns == 0) continue;
		if (int rc = fused_stage2(a, sid, n, ns, fh, ps)) return rc;
	}
	unsigned long long nh = ps.hits_seen;
	if (!ps.hits_fresh) HIP_TRY(copy_now(st, &nh, ctr() + S, sizeof(nh), hipMemcpyDeviceToHost));
	if ((int64_t)nh > fh.cap) return fail(DMND_E_NOMEM, "dmnd_seed_search: hit buffer overflow");
	c->n_seed_hits = (int64_t)nh;
	return DMND_OK;
}

// Whether a search that DMND_SEED_CHAIN does not force takes the chain (seed_chain.h). Two measured exceptions:
//  * long seeds by key class (query blocks above 2^24 positions, C5): with the chain the step went from 35.6 to 38.4-39.5 ms although
//    the seed calls got shorter -- the extension bounds that step, and a seed stage without idle gaps takes device time from it;
//  * a context whose last chain met something no buffer growth removes (deferred pairs, the tiled filter, more hits than the padded
//    sort holds: chain_rests_after) leaves the chain out for the next SEED_CHAIN_REST searches: there the chain only adds its
//    readback and an unused sort (C4, deferred pairs in every search: 9.2 ms per step this way, 9.55 with the chain tried every time).
//    (More hits than a pad below the sort's ceiling is not such a case: the next search's pad is sized for them.)
enum { SEED_CHAIN_REST = 15 };
bool chain_by_default(dmnd_ctx* c, bool classes_long)
{
	if (classes_long) return false;
	if (c->seed_chain_rest > 0) { --c->seed_chain_rest; return false; }
	return true;
}
bool chain_rests_after(const ChainPlan& plan, unsigned long long status, bool pad_grows)
{
	return plan.point == CHAIN_FROM_DEFERRED || (plan.point == CHAIN_FROM_SORT && !pad_grows) || (status & CHAIN_TILED) != 0;
}

// The padded sort runs over its whole pad whatever the hit count: the pad is sized like the readback, by the context's last hit count
// plus a quarter, here rounded up to a power of two (the sort merges in doubling runs) -- under the ceiling (SeedHooks::sort_cap), which
// also serves a context's first search. More hits than that: the host's launches sort them, and the next search's pad is sized for them.
int64_t chain_sort_pad(int64_t ceiling, int64_t last_hits)
{
	if (last_hits < 0) return ceiling;
	int64_t pad = 1024;
	while (pad < ceiling && pad < last_hits + last_hits / 4) pad <<= 1;
	return std::min(pad, ceiling);
}

// what sort_seed_hits needs to know about the blocks: the widths of the key's fields
struct HitSortBits { int query, subject, off; };
HitSortBits hit_sort_bits(dmnd_ctx* c)
{
	auto bits_of = [](uint64_t v) { int b = 1; while (b < 64 && (v >> b) != 0) ++b; return b; };
	const std::vector<int64_t>& qlim = c->limits[DMND_QUERY];
	if (c->max_query_len_generation != c->query_generation || c->max_query_len <= 0) {
		int64_t m = 1;
		for (size_t i = 0; i + 1 < qlim.size(); ++i) m = std::max(m, qlim[i + 1] - qlim[i]);
		c->max_query_len = m; c->max_query_len_generation = c->query_generation;
	}
	return HitSortBits{ bits_of((uint64_t)std::max<size_t>(qlim.size(), 2) - 1), bits_of((uint64_t)c->block_len[DMND_TARGET]), bits_of((uint64_t)c->max_query_len) };
}

// a shape's arguments on the chain: the whole shared lists (the shape's range is in the counter block), every list of phase 2
SeedArgs SeedRun::chain_args(const SeedChain& ch, int64_t def_cap, int sid) const
{
	SeedArgs a = args_with_lists(sid, ch.matched_cap, 0, ch.hit_cap, def_cap);
	a.survivors = c->seed_survivors.as<SeedSurvivor>(); a.survivor_cap = ch.survivor_cap;
	a.scored = c->seed_scored.as<SeedScored>();
	return a;
}

// ---- Chain mode (seed_chain.h; DMND_SEED_CHAIN=0/1 forces the host-driven path or the chain): everything from here to the sorted
// hits is enqueued without a host wait, one copy brings back the counters, the status word and the leading hits, and res says
// where the host-driven code continues where the status word asks for it. res.cap_total: the capacity of the joined-position lists.
int SeedRun::chain(ChainResume& res)
{
	const int64_t cap_total = res.cap_total;
	const int64_t surv_cap = cap_or(hooks.survivor_cap, std::max<int64_t>((int64_t)1 << 20, (int64_t)std::min(c->seed_survivors.cap / sizeof(SeedSurvivor), c->seed_scored.cap / sizeof(SeedScored))));
	const int64_t hit_cap = cap_or(hooks.hit_cap, std::max<int64_t>((int64_t)1 << 20, (int64_t)(c->seed_hits.cap / sizeof(dmnd_seed_hit))));
	const int64_t def_cap = cap_or(hooks.deferred_cap, std::max<int64_t>((int64_t)1 << 18, (int64_t)(c->seed_deferred.cap / sizeof(SeedDeferred))));
	const int64_t sort_ceiling = hooks.sort_cap, sort_cap = chain_sort_pad(sort_ceiling, c->seed_last_hits);
	const int64_t ret_hits = chain_ret_hits(hooks.readback_bytes, (int64_t)sizeof(dmnd_seed_hit), sort_cap);
	const size_t ret_bytes = chain_ret_header_bytes(S) + (size_t)ret_hits * sizeof(dmnd_seed_hit);
	const HitSortBits bits = hit_sort_bits(c);
	const bool one_key = sort_seed_hits_one_key(bits.query, bits.subject, bits.off);
	if (int rc = c->matched_slot.ensure((size_t)cap_total * sizeof(uint32_t))) return rc;
	if (int rc = c->matched_loc.ensure((size_t)cap_total * sizeof(int64_t))) return rc;
	if (int rc = c->seed_survivors.ensure((size_t)surv_cap * sizeof(SeedSurvivor))) return rc;
	if (int rc = c->seed_scored.ensure((size_t)surv_cap * sizeof(SeedScored))) return rc;
	if (int rc = c->seed_hits.ensure((size_t)hit_cap * sizeof(dmnd_seed_hit))) return rc;
	if (int rc = c->seed_deferred.ensure((size_t)def_cap * sizeof(SeedDeferred))) return rc;
	if (int rc = c->seed_hits_sorted.ensure((size_t)sort_ceiling * sizeof(dmnd_seed_hit))) return rc;
	for (int k = 0; k < 2; ++k) {
		if (int rc = c->sort_keys[k].ensure((size_t)sort_ceiling * sizeof(uint64_t))) return rc;
		if (int rc = c->sort_idx[k].ensure((size_t)sort_ceiling * sizeof(uint32_t))) return rc;
	}
	if (int rc = c->seed_ret.ensure(ret_bytes)) return rc;
	if (int rc = c->seed_ret_h.ensure(ret_bytes)) return rc;
	SeedChain ch;
	ch.ctr = ctr(); ch.S = S;
	ch.matched_cap = cap_total; ch.survivor_cap = surv_cap; ch.hit_cap = hit_cap; ch.tiled_from = tiled_from;
	for (int sid = 0; sid < S; ++sid) {
		const SeedArgs a = chain_args(ch, def_cap, sid);
		tm.start();
		if (int rc = query_side(a, sid, !index_ready)) return rc;
		tm.stop(c->seed_ms[0]);
		tm.start();
		HIP_TRY(stream_shape(a, sid));
		tm.stop(c->seed_ms[1]);
		HIP_TRY(launch_seed_chain_streamed(ch, sid, st));
	}
	for (int sid = 0; sid < S && sp.seed_encoding == SEED_SPACED; ++sid) {
		tm.start();
		HIP_TRY(launch_seed_chain_mask(chain_args(ch, def_cap, sid), ch, sid, st));
		tm.stop(c->seed_ms[2]);
	}
	for (int sid = 0; sid < S; ++sid) {
		tm.start();
		HIP_TRY(launch_seed_chain_shape(chain_args(ch, def_cap, sid), ch, sid, st));
		tm.stop(c->seed_ms[3]);
	}
	{
		uint64_t* keys[2] = { c->sort_keys[0].as<uint64_t>(), c->sort_keys[1].as<uint64_t>() };
		uint32_t* idx[2] = { c->sort_idx[0].as<uint32_t>(), c->sort_idx[1].as<uint32_t>() };
		HIP_TRY(launch_seed_chain_sort(ch, true, c->seed_hits.as<dmnd_seed_hit>(), c->seed_hits_sorted.as<dmnd_seed_hit>(), sort_cap, keys, idx, &c->sort_tmp, &c->sort_tmp_bytes, st,
			bits.query, bits.subject, bits.off, !sp.use_ungapped, c->seed_ret.as<char>(), ret_hits));
	}
	// the copy is on the call's serial path: of the hits that the budget allows it carries as many as the context's last search
	// found plus a quarter (more hits than that: dmnd_seed_hits copies, and the next search's readback is sized for them)
	// (dmnd_set_seed_hits_resident: none of them -- the caller reads the hits where they lie in HBM)
	const int64_t copy_hits = c->seed_hits_stay ? 0 : c->seed_last_hits < 0 ? ret_hits : std::min<int64_t>(ret_hits, c->seed_last_hits + c->seed_last_hits / 4 + 1024);
	HIP_TRY(hipMemcpyAsync(c->seed_ret_h.p, c->seed_ret.p, chain_ret_header_bytes(S) + (size_t)copy_hits * sizeof(dmnd_seed_hit), hipMemcpyDeviceToHost, st));
	lap("chain enqueued");
	{
		// the expected length of this wait: drops to a shorter wait at once, follows longer ones by an eighth per call (a call
		// that ran beside a busy extension must not make the next ones sleep through their completion)
		double d = c->seed_chain_wait_us;
		HIP_TRY(sync_stream(st, &d));
		c->seed_chain_wait_us = (c->seed_chain_wait_us <= 0.0 || d < c->seed_chain_wait_us) ? d : c->seed_chain_wait_us + (d - c->seed_chain_wait_us) / 8;
	}
	lap("chain waited for");
	pristine = false;
	const unsigned long long* ret = c->seed_ret_h.as<unsigned long long>();
	const unsigned long long status = ret[chain_ctr_status(S)], done = ret[chain_ctr_done(S)];
	for (int sid = 0; sid < S; ++sid) {
		m_off[sid] = sid ? (int64_t)ret[sid - 1] : 0;
		counts[sid] = ret[sid] - (unsigned long long)m_off[sid];
	}
	m_off[S] = (int64_t)ret[S - 1];
	const ChainPlan plan = chain_plan(status, done, S, one_key);
	chain_path_name(path, sizeof(path), plan, status);
	c->seed_trace.assign((size_t)2 * S, 0);
	for (int sid = 0; sid < S && (unsigned long long)sid < done + ((status & (CHAIN_SURVIVORS_OVER | CHAIN_HITS_OVER | CHAIN_DEFERRED)) ? 1 : 0); ++sid) c->seed_trace[sid] = ret[chain_ctr_survivors_of(S) + sid];
	if (hooks.chain < 0 && chain_rests_after(plan, status, one_key && (int64_t)ret[S] <= sort_ceiling)) c->seed_chain_rest = SEED_CHAIN_REST;
	res = chain_resume(plan, ret, S, cap_total, hit_cap, def_cap);
	if (res.dirty) {
		for (int k = 0; k < 3; ++k) tm.discard(&c->seed_ms[k]);      // the abandoned attempt does not count
		if (hooks.trace) std::fprintf(stderr, "dmnd_seed_search: joined-position buffer overflow, %lld positions against a capacity of %lld: phase 1 runs again\n", (long long)m_off[S], (long long)cap_total);
	}
	if (res.discard_pairs_time) tm.discard(&c->seed_ms[3]);
	if (plan.point == CHAIN_FROM_DEFERRED) c->seed_trace[S + plan.shape] = res.deferred_n;
	if (res.hits_done) {
		c->n_seed_hits = (int64_t)ret[S];
		if (c->n_seed_hits <= copy_hits) { c->seed_ret_hits = c->n_seed_hits; c->seed_ret_bytes_header = chain_ret_header_bytes(S); }
	}
	return DMND_OK;
}

// phase 1: index + stream + mask, every shape. The joined-position lists of all shapes share one buffer, which grows on overflow.
int SeedRun::phase1(const ChainResume& res)
{
	int64_t cap_total = res.cap_total;
	for (int attempt = 0;; ++attempt) {
		if (int rc = c->matched_slot.ensure((size_t)cap_total * sizeof(uint32_t))) return rc;
		if (int rc = c->matched_loc.ensure((size_t)cap_total * sizeof(int64_t))) return rc;
		if (attempt > 0 || res.dirty) {
			HIP_TRY(hipMemsetAsync(c->counters.p, 0, (size_t)(S + 8) * sizeof(unsigned long long), st));
			HIP_TRY(hipMemsetAsync(c->seed_keys.p, 0xff, (size_t)S * slot_bytes, st));
			HIP_TRY(hipMemsetAsync(c->seed_bitmap.p, 0, z.bm_total, st));
		}
		bool overflow = false;
		int64_t off = 0;
		for (int sid = 0; sid < S; ++sid) {
			m_off[sid] = off;
			// after an overflow the remaining shapes only count (capacity 0): a negative capacity would pass the kernels' unsigned bound test
			SeedArgs a = args_for(sid, std::max<int64_t>(cap_total - off, 0), std::min(off, cap_total));
			tm.start();
			if (int rc = query_side(a, sid, !index_ready || attempt > 0 || res.dirty)) return rc;
			tm.stop(c->seed_ms[0]);
			tm.start();
			HIP_TRY(stream_shape(a, sid));
			tm.stop(c->seed_ms[1]);
			HIP_TRY(copy_now(st, &counts[sid], a.matched_count, sizeof(unsigned long long), hipMemcpyDeviceToHost));
			if ((int64_t)counts[sid] > cap_total - off) overflow = true;
			off += (int64_t)counts[sid];
		}
		m_off[S] = off;
		if (!overflow) break;
		if (attempt >= 2) return fail(DMND_E_NOMEM, "dmnd_seed_search: joined-position buffer overflow");
		if (hooks.trace) std::fprintf(stderr, "dmnd_seed_search: joined-position buffer overflow, %lld positions against a capacity of %lld: phase 1 runs again\n", (long long)off, (long long)cap_total);
		cap_total = off + off / 8 + 1024;
	}
	// Search::mask_seeds (per joined group) only exists for spaced seeds; the query-indexed mode masked at enumeration
	for (int sid = 0; sid < S && sp.seed_encoding == SEED_SPACED; ++sid) {
		SeedArgs a = args_for(sid, (int64_t)counts[sid], m_off[sid]);
		tm.start();
		HIP_TRY(launch_seed_mask(a, sid, st, (int64_t)counts[sid]));
		tm.stop(c->seed_ms[2]);
	}
	return DMND_OK;
}

// DMND_TRACE: the seed pairs of the joined positions, for the summary line
int SeedRun::count_pairs()
{
	pristine = false;
	HIP_TRY(hipMemsetAsync(ctr() + S + 3, 0, sizeof(unsigned long long), st));
	for (int sid = 0; sid < S; ++sid) {
		SeedArgs a = args_for(sid, (int64_t)counts[sid], m_off[sid]);
		HIP_TRY(launch_seed_count_pairs(a, (int64_t)counts[sid], ctr() + S + 3, st));
	}
	HIP_TRY(copy_now(st, &n_pairs, ctr() + S + 3, sizeof(n_pairs), hipMemcpyDeviceToHost));
	return DMND_OK;
}

// one shape of phase 2: (sort and tiled, or plain) Hamming filter -> survivor list -> stage-2 kernels
int SeedRun::pair_filter(SeedArgs& a, int sid)
{
	const int64_t n = (int64_t)counts[sid];
	// many joined positions (short seeds): sort them by seed and run the LDS-tiled filter; otherwise one thread per position
	const bool tiled = n >= tiled_from;
	if (hooks.trace && tiled) std::fprintf(stderr, "dmnd_seed_search: shape %d, %llu joined positions: sorted by seed, tiled pair filter\n", sid, counts[sid]);
	if (tiled) {
		if (int rc = c->seed_slot2.ensure((size_t)n * sizeof(uint32_t))) return rc;
		if (int rc = c->seed_loc2.ensure((size_t)n * sizeof(int64_t))) return rc;
		HIP_TRY(sort_matched_by_slot(a.matched_slot, c->seed_slot2.as<uint32_t>(), a.matched_loc, c->seed_loc2.as<int64_t>(), n, slot_bits,
			&c->sort_tmp, &c->sort_tmp_bytes, st));
		a.matched_slot = c->seed_slot2.as<uint32_t>(); a.matched_loc = c->seed_loc2.as<int64_t>();      // also for the deferred pass behind it
	}
	int64_t surv_cap = cap_or(hooks.survivor_cap, std::max<int64_t>(std::max<int64_t>((int64_t)1 << 20, tiled ? 2 * n : n), (int64_t)(c->seed_survivors.cap / sizeof(SeedSurvivor))));
	unsigned long long ns = 0;
	for (int pass = 0;; ++pass) {
		if (int rc = c->seed_survivors.ensure((size_t)surv_cap * sizeof(SeedSurvivor))) return rc;
		a.survivors = c->seed_survivors.as<SeedSurvivor>(); a.survivor_cap = surv_cap;
		if (!pristine || pass > 0) HIP_TRY(hipMemsetAsync(a.survivor_count, 0, sizeof(unsigned long long), st));
		if (tiled) HIP_TRY(launch_seed_pairs_tiled(a, sid, n, st));
		else HIP_TRY(launch_seed_pairs(a, sid, n, st));
		HIP_TRY(hipMemcpyAsync(&ns, a.survivor_count, sizeof(ns), hipMemcpyDeviceToHost, st));
		HIP_TRY(sync_stream(st));
		if ((int64_t)ns <= surv_cap) break;
		if (pass >= 2) return fail(DMND_E_NOMEM, "dmnd_seed_search: survivor buffer overflow");
		surv_cap = (int64_t)ns + 1024;
	}
	c->seed_trace[sid] = ns;
	if (int rc = c->seed_scored.ensure((size_t)std::max<unsigned long long>(ns, 1) * sizeof(SeedScored))) return rc;
	a.scored = c->seed_scored.as<SeedScored>();
	HIP_TRY(launch_seed_post(a, sid, (int64_t)ns, st, !pristine));
	pristine = false;                                  // from here on the counters hold this shape's numbers
	return DMND_OK;
}

// phase 2: pair filter per shape; hit and deferred-pair buffers grow on overflow. res: what a chain left to do, and to keep
int SeedRun::phase2(const ChainResume& res)
{
	int64_t hit_cap = cap_or(hooks.hit_cap, std::max<int64_t>(std::max<int64_t>((int64_t)1 << 20, m_off[S] / 8), (int64_t)(c->seed_hits.cap / sizeof(dmnd_seed_hit))));
	int64_t def_cap = cap_or(hooks.deferred_cap, std::max<int64_t>((int64_t)1 << 18, (int64_t)(c->seed_deferred.cap / sizeof(SeedDeferred))));
	// the continuation of a chain: the hits (and deferred pairs) it left stay where they are, or the buffer that overflowed has grown
	if (res.p2_keep) { hit_cap = res.hit_cap; def_cap = res.def_cap; }
	else { hit_cap = std::max(hit_cap, res.hit_cap); def_cap = std::max(def_cap, res.def_cap); }
	for (int attempt = 0;; ++attempt) {
		const bool keep = attempt == 0 && res.p2_keep;
		if (int rc = c->seed_hits.ensure((size_t)hit_cap * sizeof(dmnd_seed_hit))) return rc;
		if (int rc = c->seed_deferred.ensure((size_t)def_cap * sizeof(SeedDeferred))) return rc;
		if (!pristine && !keep) HIP_TRY(hipMemsetAsync(ctr() + S, 0, sizeof(unsigned long long), st));
		if (attempt > 0) tm.discard(&c->seed_ms[3]);
		PostState ps;
		if (!keep) c->seed_trace.assign((size_t)2 * S, 0);
		if (keep && res.deferred_sid >= 0) {
			const int sid = res.deferred_sid;
			SeedArgs a = args_with_lists(sid, (int64_t)counts[sid], m_off[sid], hit_cap, def_cap);
			tm.start();
			if (int rc = seed_deferred_pass(c, a, sid, (int64_t)counts[sid], (int64_t)res.deferred_n, st)) return rc;
			tm.stop(c->seed_ms[3]);
		}
		for (int sid = keep ? res.p2_first : 0; sid < S; ++sid) {
			SeedArgs a = args_with_lists(sid, (int64_t)counts[sid], m_off[sid], hit_cap, def_cap);
			if (!pristine) {
				SeedClear clr;
				clr.add(a.deferred_count, 2 * sizeof(unsigned long long), 0);
				clr.add(a.need_bits, (size_t)(z.slots / 32) * sizeof(uint32_t), 0);
				HIP_TRY(launch_seed_clear(clr, st));
			}
			tm.start();
			if (int rc = pair_filter(a, sid)) return rc;
			tm.stop(c->seed_ms[3]);
			if (int rc = after_post(a, sid, (int64_t)counts[sid], def_cap, ps)) return rc;
		}
		const bool def_overflow = (int64_t)ps.def_max > def_cap;
		unsigned long long nh = ps.hits_seen;
		if (!ps.hits_fresh) HIP_TRY(copy_now(st, &nh, ctr() + S, sizeof(nh), hipMemcpyDeviceToHost));
		if ((int64_t)nh <= hit_cap && !def_overflow) { c->n_seed_hits = (int64_t)nh; break; }
		if (attempt >= 3) return fail(DMND_E_NOMEM, "dmnd_seed_search: hit buffer overflow");
		if ((int64_t)nh > hit_cap) hit_cap = (int64_t)nh + 1024;
		if (def_overflow) def_cap = (int64_t)ps.def_max + 1024;
	}
	return DMND_OK;
}

// order the hits by (query, subject, seed_offset, score) on the device: what align_queries needs (hits grouped by query),
// made deterministic (the append order of the kernels is not)
int SeedRun::sort_hits()
{
	const int64_t n = c->n_seed_hits;
	if (n > 0xffffffffLL) return fail(DMND_E_CAP, "dmnd_seed_search: more than 2^32 seed hits in one block pair");
	if (int rc = c->seed_hits_sorted.ensure((size_t)n * sizeof(dmnd_seed_hit))) return rc;
	if (int rc = c->sort_keys[0].ensure((size_t)n * sizeof(uint64_t))) return rc;
	if (int rc = c->sort_keys[1].ensure((size_t)n * sizeof(uint64_t))) return rc;
	if (int rc = c->sort_idx[0].ensure((size_t)n * sizeof(uint32_t))) return rc;
	if (int rc = c->sort_idx[1].ensure((size_t)n * sizeof(uint32_t))) return rc;
	uint64_t* keys[2] = { c->sort_keys[0].as<uint64_t>(), c->sort_keys[1].as<uint64_t>() };
	uint32_t* idx[2] = { c->sort_idx[0].as<uint32_t>(), c->sort_idx[1].as<uint32_t>() };
	const HitSortBits bits = hit_sort_bits(c);
	HIP_TRY(sort_seed_hits(c->seed_hits.as<dmnd_seed_hit>(), c->seed_hits_sorted.as<dmnd_seed_hit>(), n, keys, idx, &c->sort_tmp, &c->sort_tmp_bytes, st,
		bits.query, bits.subject, bits.off, !sp.use_ungapped));
	HIP_TRY(sync_stream(st));
	return DMND_OK;
}

// DMND_TRACE: the summary line (it ends with the path), and a line of its own on which stream ran and what this call did about the
// reference cache
void SeedRun::trace_summary() const
{
	std::fprintf(stderr, "dmnd_seed_search: %d shapes, %lld query positions, joined reference positions per shape:", S, (long long)nq_pos);
	for (int sid = 0; sid < S; ++sid) std::fprintf(stderr, " %llu", counts[sid]);
	std::fprintf(stderr, " | pairs %llu | Hamming survivors:", n_pairs);
	for (int sid = 0; sid < S && (size_t)sid < c->seed_trace.size(); ++sid) std::fprintf(stderr, " %llu", c->seed_trace[sid]);
	std::fprintf(stderr, " | deferred:");
	for (int sid = 0; sid < S && (size_t)(S + sid) < c->seed_trace.size(); ++sid) std::fprintf(stderr, " %llu", c->seed_trace[S + sid]);
	std::fprintf(stderr, " | hits %lld | ms index %.2f stream %.2f mask %.2f pairs %.2f | path: %s\n", (long long)c->n_seed_hits, c->seed_ms[0], c->seed_ms[1], c->seed_ms[2], c->seed_ms[3], path);
	const size_t held = c->seed_ref_codes.cap + c->seed_ref_lists.cap + c->seed_ref_hashes.cap + c->seed_ref_counts.cap;
	if (ref_use == SEED_REF_NONE) std::fprintf(stderr, "dmnd_seed_search: stream: plain, reference cache: none, %zu bytes held\n", held);
	else std::fprintf(stderr, "dmnd_seed_search: stream: slices (%d x %g KB), reference cache: %s, %zu bytes held\n", 1 << slice_bits, (double)(z.bm1_words >> slice_bits) * 4 / 1024, ref_use == SEED_REF_BUILT ? "built" : "kept", held);
}

}

extern "C" int dmnd_seed_search(dmnd_ctx* c, const dmnd_seed_params* params, int64_t* n_hits)
{
	if (!c || !params || !n_hits) return fail(DMND_E_ARG, "dmnd_seed_search: NULL argument");
	SeedRun r(c, seed_hooks());                          // (starts the lap clock)
	*n_hits = 0;
	c->n_seed_hits = 0;                                  // a failed or empty search must not leave the previous search's hits behind
	c->seed_ret_hits = -1;
	const std::vector<int64_t>& ql = c->limits[DMND_QUERY];
	const std::vector<int64_t>& tl = c->limits[DMND_TARGET];
	if (ql.size() < 2 || tl.size() < 2) return fail(DMND_E_ARG, "dmnd_seed_search: both blocks must be uploaded with limits");
	std::memcpy(&r.sp, params, sizeof(r.sp));
	if (int rc = seed_check_params(r.sp)) return rc;
	if (int rc = r.check_blocks()) return rc;
	HIP_TRY(hipSetDevice(c->device));
	r.q_begin = ql.front(); r.q_end = ql.back(); r.t_begin = tl.front(); r.t_end = tl.back();
	r.nq_pos = r.q_end - r.q_begin; r.n_targets = (int64_t)tl.size() - 1;
	if (r.nq_pos <= 0 || r.t_end <= r.t_begin) return DMND_OK;
	if (int rc = r.geometry()) return rc;
	r.ref_decide();
	if (int rc = r.prepare()) return rc;
	if (int rc = r.ref_cache()) return rc;
	if (c->soft_valid[DMND_QUERY]) HIP_TRY(launch_seed_soft_time(r.args_for(0, 0, 0), r.st));
	ChainResume res;                                     // without a chain: the host-driven phases from their beginning
	if (r.z.fused) {
		if (int rc = r.fused()) return rc;
	}
	else {
		// start from what earlier calls already grew the buffers to: a repeated search of the same scale never takes the overflow path
		res.cap_total = cap_or(r.hooks.matched_cap, std::max<int64_t>(std::max<int64_t>((int64_t)1 << 22, 4 * r.nq_pos), (int64_t)std::min(c->matched_loc.cap / sizeof(int64_t), c->matched_slot.cap / sizeof(uint32_t))));
		if (r.hooks.chain >= 0 ? r.hooks.chain != 0 : chain_by_default(c, r.classes_long))
			if (int rc = r.chain(res)) return rc;
		if (res.phase1_again)
			if (int rc = r.phase1(res)) return rc;
		if (r.hooks.trace)
			if (int rc = r.count_pairs()) return rc;
		r.lap("phase 1 done (index, stream, mask of every shape)");
		if (!res.hits_done)
			if (int rc = r.phase2(res)) return rc;
	}
	r.lap("filters done");
	if (r.z.reuse) c->qindex_signature = r.signature;    // every shape's query side is complete and resident
	if (c->n_seed_hits > 0 && !res.hits_done)
		if (int rc = r.sort_hits()) return rc;
	r.lap("hits sorted");
	if (r.phases) {
		unsigned long long t[8];
		HIP_TRY(copy_now(r.st, t, r.ctr() + r.S + 8, sizeof(t), hipMemcpyDeviceToHost));
		std::fprintf(stderr, "SEED_PHASES (ms of workgroup time, summed): start %.1f | windows %.1f | level 1 %.1f | table %.1f | light lists %.1f | heavy lists %.1f\n",
			t[0] / 1e5, t[1] / 1e5, t[2] / 1e5, t[3] / 1e5, t[4] / 1e5, t[5] / 1e5);
	}
	r.tm.collect();
	c->seed_ms[4] = c->seed_ms[0] + c->seed_ms[1] + c->seed_ms[2] + c->seed_ms[3];
	if (r.hooks.trace) r.trace_summary();
	*n_hits = c->n_seed_hits;
	c->seed_last_hits = c->n_seed_hits;
	c->seed_last_joined = 0;
	for (int sid = 0; sid < r.S; ++sid) c->seed_last_joined += (int64_t)r.counts[sid];
	return DMND_OK;
}

extern "C" int64_t dmnd_seed_hit_count(const dmnd_ctx* c) { return c ? c->n_seed_hits : -1; }

extern "C" int dmnd_set_seed_hits_resident(dmnd_ctx* c, int on)
{
	if (!c) return fail(DMND_E_ARG, "dmnd_set_seed_hits_resident: ctx is NULL");
	c->seed_hits_stay = on != 0;
	return DMND_OK;
}

extern "C" int dmnd_seed_hits(dmnd_ctx* c, dmnd_seed_hit* out, int64_t cap)
{
	if (!c || (!out && c->n_seed_hits > 0)) return fail(DMND_E_ARG, "dmnd_seed_hits: NULL argument");
	if (cap < c->n_seed_hits) return fail(DMND_E_CAP, "dmnd_seed_hits: buffer too small");
	if (c->n_seed_hits == 0) return DMND_OK;
	// chain mode: the hits came back with the search's one copy where they fit its byte budget
	if (c->seed_ret_hits == c->n_seed_hits && c->seed_ret_h.p) {
		std::memcpy(out, c->seed_ret_h.as<char>() + c->seed_ret_bytes_header, (size_t)c->n_seed_hits * sizeof(dmnd_seed_hit));
		return DMND_OK;
	}
	HIP_TRY(hipSetDevice(c->device));
	if (int rc = download_bytes(c, out, c->seed_hits_sorted.p, (size_t)c->n_seed_hits * sizeof(dmnd_seed_hit))) return rc;      // sorted by dmnd_seed_search
	return DMND_OK;
}
