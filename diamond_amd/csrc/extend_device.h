// extend_device.h -- the device half of dmnd_extend as extend_host.hip calls it (extend_device.hip; round 6): the planner over the
// call's seed hits (plan_kernels.hip) and the extension of the planned queries in HBM (extend_kernels.hip).
#pragma once
#include <stdint.h>
#include <vector>
#include "ctx.h"
#include "plan_kernels.h"
#include "filter_core.h"

namespace dmnd {

struct CbsModel;

// what the two halves need of the call's configuration (extend_host.hip HostCfg)
struct DeviceCfg {
	int gap_open = 11, gap_extend = 1;
	int band_mode_fast = 1;              // Extension::Mode::BANDED_FAST
	int max_target_seqs = 25;
	int64_t ranking_chunk = 128;         // ranking_chunk_size (extend.cpp:79-92)
	int64_t max_swipe_dp = 1000000;
	bool use_cbs = true;                 // Hauser bias
	double max_evalue = 0.001;
	double min_bit_score = 0.0;          // --min-score
	FilterCfg filters;                   // --id, --approx-id, --query-cover, --subject-cover (filter_core.h)
	double top = -1.0;                   // --top: >= 0 = the targets within this percentage of the best bit score, -k plays no part
	int contexts = 1;                    // 6: translated queries -- the planner groups per read, the records carry the winning frame
	bool ext_full = false;               // Extension::Mode::FULL: one full-matrix DpTarget per (context, target) unit with a hit (plan_full_kernel); max_swipe_dp is held against query length x target length
	int cbs_mode = 1;                    // --comp-based-stats; 2 - 5 with cbs_model: the device half adjusts the matrix of every (query, target) pair it sweeps (cbs_kernels.hip)
	const CbsModel* cbs_model = nullptr;
	int global_ranking = 0;            // > 0: the final pass of --global-ranking -- one hit per ranked target, at most this many per query, ONE ranking chunk of that size (extend.cpp:80)
};

// What the device planner hands over (page-locked host copies of its lists; valid until the context's next dmnd_extend)
struct DevPlan {
	const PlanGroup* groups = nullptr;        // translated queries: the (read, target) pairs (PlanArgs::pairs), n_groups of them
	const PlanQuery* queries = nullptr;       // n_queries + 1 entries
	const PlanBand* bands = nullptr;
	const uint32_t* band_query = nullptr;     // translated queries: the context of every band, and per group (= pair) the ungapped score of context 0
	const uint16_t* ungapped0 = nullptr;
	uint32_t n_groups = 0, n_queries = 0, n_bands = 0, n_on_host = 0;
	uint32_t n_chain = 0, n_chain_big = 0, n_relisted = 0;      // PlanCounters: the two chaining lists as the kernels left them
	bool unsorted = false;                    // the hits were not in (query, location, seed offset) order: nothing was planned
	PlanArgs dev;                             // the same lists (and the planner's inputs) where they lie in HBM
};

// Runs the planner over the call's hits (in c->xd_hits, with their x-drop extensions in c->xd_out -- not read in Mode::FULL -- and
// -- gf_on -- their gapped filter flags in c->gf_flags), waits for it and leaves its lists in HBM. planned = false: the hits are not in
// (query, location, seed offset) order, the host has to plan.
int plan_on_device(dmnd_ctx* c, const DeviceCfg& h, int64_t n_hits, bool gf_on, DevPlan& plan, bool& planned);
// The planner's lists on the host (page-locked copies, valid until the context's next dmnd_extend): only the host path reads them
int plan_fetch_lists(dmnd_ctx* c, DevPlan& plan);
// The extension of the planned queries in HBM, from the planner's bands to the match records (extend_kernels.h). records: those
// queries' matches in output order with the HOST's e-value and bit score; qstate[k] (k = index into plan.queries): EXT_Q_DEVICE =
// done here, anything else = the host path has to extend the query. done = false: nothing was done here, every query goes to the host path.
// transcript != NULL: the caller's transcript arena of transcript_cap bytes. The records' packed transcripts (transcript_len bytes
// and a 0 terminator each) are written to it from offset 0 on in record order, hsp.transcript_off of each record points at its own,
// *transcript_used = their bytes; more than transcript_cap: DMND_E_CAP, nothing written. The records then do not stay in HBM for a
// join (c->ext_records_dev stays NULL). transcript == NULL: no transcripts, hsp.transcript_off = -1.
// qdata / tdata: the caller's blocks; read only with h.cbs_model, for the pairs the adjustment kernel hands back to the host form.
int extend_on_device(dmnd_ctx* c, const DeviceCfg& h, const DevPlan& plan, int threads, std::vector<dmnd_match>& records, std::vector<uint8_t>& qstate, bool& done,
	uint8_t* transcript = nullptr, int64_t transcript_cap = 0, int64_t* transcript_used = nullptr, const int8_t* qdata = nullptr, const int8_t* tdata = nullptr);

}  // namespace dmnd
