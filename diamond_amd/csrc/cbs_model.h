// cbs_model.h -- the device form's view of a CbsModel (cbs_adjust.h -> cbs_core.h): the tables the kernel reads, the guard
// widths and the iteration cap. Shared by the launcher (cbs_kernels.hip) and the lane emulator.
#pragma once
#include <cstring>
#include "cbs_adjust.h"
#include "cbs_core.h"

namespace dmnd {

// max_its <= 0: the built-in cap; never above the host's own limit
inline void cbs_dev_model(CbsDevModel& d, const CbsModel& m, int mode, int max_its)
{
	std::memcpy(d.joint_probs, m.joint_probs, sizeof d.joint_probs);
	std::memcpy(d.background, m.background, sizeof d.background);
	std::memcpy(d.matrix8, m.matrix8, sizeof d.matrix8);
	d.lambda = m.ideal_lambda / m.scale;
	d.err_tolerance = m.err_tolerance; d.angle = m.angle;
	d.distance_threshold = m.distance_threshold; d.length_ratio_threshold = m.length_ratio_threshold;
	d.eps_round = CBS_EPS_ROUND; d.eps_norm = CBS_EPS_NORM; d.eps_angle = CBS_EPS_ANGLE;
	d.mode = mode; d.scale = m.scale; d.pad = 0;
	d.max_its = max_its > 0 ? max_its : CBS_DEVICE_MAX_ITS;
	if (d.max_its > m.it_limit) d.max_its = m.it_limit;
}

}  // namespace dmnd
