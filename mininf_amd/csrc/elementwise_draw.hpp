// The one-noise-word draws of the discrete and heavy-tailed families, shared by the predictive
// sites (predictive.hip) and the guide factors (elementwise_guide.hip): one definition, so a draw
// is the same function of its parameters and its noise word in both.
#pragma once

#include "common.hpp"

namespace mi {

// The largest float below 1: what the top grid point of u01, (2^24 - 1/2) 2^-24, which rounds to
// 1.0f, is read as where u = 1 is a pole or gives a draw outside the support.
constexpr float kBelowOne = 0.99999994f;

// One draw from its noise word: `v` is the element's uniform (u01) or, for the two normal-based
// families, its standard normal.
template <int FAMILY>
MI_DEV float pred_draw(float a, float b, float v) {
  if (FAMILY == MI_PRED_BERNOULLI_PROBS) return v < a ? 1.0f : 0.0f;
  if (FAMILY == MI_PRED_BERNOULLI_LOGITS) return v < 1.0f / (1.0f + expf(-a)) ? 1.0f : 0.0f;
  if (FAMILY == MI_PRED_EXPONENTIAL) return -logf(v) / a;
  // The top grid point (2^24 - 1/2) 2^-24 rounds to 1.0f, the pole of the three draws below:
  // they read it as the largest float below 1, so their upper tail stops at the 2^-24 quantile.
  if (FAMILY == MI_PRED_LAPLACE || FAMILY == MI_PRED_CAUCHY || FAMILY == MI_PRED_HALF_CAUCHY)
    v = fminf(v, kBelowOne);
  if (FAMILY == MI_PRED_LAPLACE) {
    const float d = v - 0.5f;   // exact: v is on the 24-bit grid
    return a - b * copysignf(1.0f, d) * log1pf(-2.0f * fabsf(d));
  }
  if (FAMILY == MI_PRED_CAUCHY) {
    // tan(pi (u - 1/2)) from sin and cos of the exact half-turn fraction: no rounding of the
    // argument, so the result stays accurate up to the last grid point before the pole
    float s, c;
    sincospif(v - 0.5f, &s, &c);
    return fmaf(b, s / c, a);
  }
  if (FAMILY == MI_PRED_HALF_CAUCHY) {
    float s, c;
    sincospif(0.5f * v, &s, &c);
    return a * (s / c);
  }
  if (FAMILY == MI_PRED_HALF_NORMAL) return a * fabsf(v);
  return expf(fmaf(v, b, a));   // MI_PRED_LOG_NORMAL
}

constexpr bool pred_normal_based(int family) {
  return family == MI_PRED_HALF_NORMAL || family == MI_PRED_LOG_NORMAL;
}

constexpr bool pred_two_parameters(int family) {
  return family == MI_PRED_LAPLACE || family == MI_PRED_CAUCHY || family == MI_PRED_LOG_NORMAL;
}

// The noise word as a guide factor reads it: every uniform family takes u = 1.0f as 1 - 2^-24.
// For the three pole families that is pred_draw's own clamp; the Exponential's -log(1) / rate = 0
// would lie outside the support of whatever site reads the draw.
template <int FAMILY>
MI_DEV float guide_noise(float v) {
  return pred_normal_based(FAMILY) ? v : fminf(v, kBelowOne);
}

// d draw / d a and d draw / d b of pred_draw at the guide's noise word v (guide_noise applied).
// With t the standardised draw (loc 0, scale 1):
//   LogNormal   d/dloc = z, d/dscale = z eps        Laplace, Cauchy  d/dloc = 1, d/dscale = t
//   HalfCauchy, HalfNormal  d/dscale = t            Exponential      d/drate = log(u) / rate^2
template <int FAMILY>
MI_DEV void guide_draw_factors(float a, float b, float v, float& fa, float& fb) {
  fb = 0.0f;
  if (FAMILY == MI_PRED_LOG_NORMAL) {
    fa = pred_draw<FAMILY>(a, b, v);
    fb = fa * v;
  } else if (FAMILY == MI_PRED_LAPLACE || FAMILY == MI_PRED_CAUCHY) {
    fa = 1.0f;
    fb = pred_draw<FAMILY>(0.0f, 1.0f, v);
  } else if (FAMILY == MI_PRED_EXPONENTIAL) {
    fa = logf(v) / (a * a);
  } else {   // HalfCauchy, HalfNormal
    fa = pred_draw<FAMILY>(1.0f, 0.0f, v);
  }
}

}  // namespace mi
