// pool_plan.h -- the host side of a pooled ragged call (text embeddings): where its rows go and what pool.hip's workgroups are told.
// Built by ONE function, pool_plan() in backend_rows.hip, from the ragged step's own planner: nano_hip_step_rows_pool,
// nano_hip_op_pool_rows and the query nano_hip_rows_pool_plan all go through it.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/nano_mi355x.h"

namespace nano {

#pragma GCC visibility push(hidden)
struct PoolPlan {
    std::vector<uint32_t> pass_start, where;               // pass p feeds rows pass_start[p] .. pass_start[p + 1] - 1; caller row r is fed as row where[r]
    std::vector<uint32_t> row_seg, row_ordinal;            // per fed row: its segment; its ordinal among the segment's pooled rows (0xffffffff: not pooled)
    std::vector<uint32_t> group_start;                     // pass p's workgroups are groups group_start[p] .. group_start[p + 1] - 1
    std::vector<uint32_t> map;                             // the device image: POOL_GROUP_WORDS words per group (kernels.h), then the groups' row lists
    uint32_t n_groups() const { return group_start.empty() ? 0u : group_start.back(); }
    uint32_t n_passes() const { return (uint32_t)group_start.size() - 1u; }
};
// NANO_HIP_EINVAL as nano_hip_rows_plan, and for pooling > NANO_POOL_MEAN
int pool_plan(const NanoHipRowSeg *segs, uint32_t n_segs, uint32_t cap, uint32_t max_seq_len, uint32_t pooling, PoolPlan *out);
#pragma GCC visibility pop

}  // namespace nano
