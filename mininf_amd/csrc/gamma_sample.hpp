// The standard-Gamma sampler of the guide kernels and its Philox sub-stream, shared by the Beta /
// Gamma samplers (guide.hip) and the Dirichlet sampler (dirichlet.hip): one definition, so a
// variate is the same function of (seed, step, stream, sub-stream, element, particle) in all of
// them.
#pragma once

#include "common.hpp"

namespace mi {

// -------------------------------------------------------------------------------------------------
// Marsaglia-Tsang gamma variates (G. Marsaglia, W. W. Tsang, "A simple method for generating gamma
// variables", ACM TOMS 26(3), 2000), with the alpha < 1 boost G(alpha) = G(alpha + 1) * U^(1/alpha).
// -------------------------------------------------------------------------------------------------
struct Stream {
  uint64_t seed, step;
  uint32_t stream_id, sub;
  uint64_t elem, particle;
  uint32_t block = 0;
  U4 bits{};
  int used = 4;
  MI_DEV uint32_t next() {
    if (used == 4) {
      U4 c{(uint32_t)elem, (uint32_t)particle, (uint32_t)step ^ (uint32_t)(step >> 32),
           (stream_id << 8) | (sub << 6) | (block & 63u)};
      bits = philox4x32<kGuideRounds>(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      ++block;
      used = 0;
    }
    const uint32_t out = used == 0 ? bits.x : used == 1 ? bits.y : used == 2 ? bits.z : bits.w;
    ++used;
    return out;
  }
  MI_DEV float uniform() { return u01(next()); }
  MI_DEV float normal() {
    float a, b;
    box_muller(next(), next(), a, b);
    return a;
  }
};

MI_DEV float sample_gamma(float alpha, Stream& rng) {
  float boost = 1.0f;
  if (!(alpha > 0.0f)) return 0.0f;
  if (alpha < 1.0f) {
    boost = powf(rng.uniform(), 1.0f / alpha);
    alpha += 1.0f;
  }
  const float d = alpha - 1.0f / 3.0f;
  const float c = 1.0f / sqrtf(9.0f * d);
  for (int attempt = 0; attempt < 64; ++attempt) {
    float x, y;
    int tries = 0;
    do {
      x = rng.normal();
      y = 1.0f + c * x;
    } while (y <= 0.0f && ++tries < 16);
    if (y <= 0.0f) continue;
    const float v = y * y * y;
    const float u = rng.uniform();
    const float xx = x * x;
    if (u < 1.0f - 0.0331f * xx * xx) return boost * d * v;
    if (logf(u) < 0.5f * xx + d * (1.0f - v + logf(v))) return boost * d * v;
  }
  return boost * d;  // not reached in practice (acceptance > 95 % per attempt)
}

}  // namespace mi
