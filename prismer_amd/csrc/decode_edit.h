// Shared by beam.hip and sample.hip: the arithmetic of ph_beam_topk_edit / ph_sample_step_edit on one value.
#pragma once
#include "common.h"

// transformers' RepetitionPenaltyLogitsProcessor on one value: x * theta below zero, the IEEE quotient x / theta otherwise (no reciprocal);
// the product is rounded on its own, never contracted into an add that follows it
__device__ __forceinline__ float penalised(float x, float theta) {
#pragma clang fp contract(off)
  return x < 0.f ? x * theta : x / theta;
}
