#pragma once
// mcq_classify.hpp -- what the other units need of the classify unit (mcq_classify.hip): the taxonomy handle, and the
// shared error text of mcq_last_error, which every unit sets through mcq::set_error.
#include <stdint.h>

#include "../../include/mcq.h"

struct mcq_taxonomy {
    int device;
    uint32_t n_taxa;
    uint32_t* lineage;            // device [n_taxa * 21]
    uint8_t* rank;                // device [n_taxa]
    uint32_t grid[17];            // resident workgroups of the classify kernel on this device, per max_cand
};

namespace mcq {
// sets the text mcq_last_error returns (defined in mcq_engine.hip) and returns code
__attribute__((visibility("hidden"))) int set_error(int code, const char* msg);
// checks mcq_classify_opts (shared by mcq_classify and mcq_ws_set_classify)
__attribute__((visibility("hidden"))) int check_classify_opts(const mcq_classify_opts* o);
}  // namespace mcq
