// Host side of zm_tracedcost_t (traced_cost.hip) that other translation units call: the descriptor check of every entry that takes one.
#pragma once
#include "../../include/zopt_amd.h"

namespace zm {

// sizes, counts, pointers and masks of a recorded cost; ZM_OK or an error set with set_error under the name `who`.  Host code only.
int tracedcost_check(const zm_tracedcost_t* tcost, const char* who);

}  // namespace zm
