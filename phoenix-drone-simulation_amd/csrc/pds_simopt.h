// pds_simopt.h -- launch interface of the fused sim-opt objective (csrc/pds_simopt.hip; entry point pds_simopt_evaluate in
// csrc/pds_api.hip).
#pragma once
#include "pds_types.h"

namespace pds {

struct SimoptArgs {
  Consts k;                // of the handle: model constants, dt, aggregate_phy_steps
  double time_step, G;     // float64 inputs of update_motor_dynamics (envs/agents.py:208-224)
  double gamma;
  const float *params;     // [P, 3] thrust_to_weight_ratio, motor_time_constant, latency
  const int32_t *lat_steps;  // [P] buf_size of every candidate (0: latency off)
  const float4 *acts;      // [T][M]
  const float4 *obs;       // [T][3][M]; row 0: the state the sample starts from, rows 1..T-1: the logged targets
  const float4 *pre;       // [pre_steps][M]
  int P, M, T, pre_steps;
  float *loss;             // [P, M]
  float *score;            // [P]
  float *sim_obs;          // [T - 1, P, M, 13] or nullptr
};

void launch_simopt(const SimoptArgs &a, hipStream_t s);

}  // namespace pds
