// seed_ref_state.h -- what a context remembers about its reference-side seed cache (seed_slices_core.h): the key it was built or last
// asked for, as bytes, and how far it got. On its own so that ctx.h needs none of the seed stage's headers.
#pragma once
#include <string>

namespace dmnd {

struct SeedRefState {
	std::string key;                     // a SeedRefKey's bytes
	int seen = 0;                        // 0: nothing; 1: key was searched once, nothing built; 2: the cache holds key's routing
};

}  // namespace dmnd
