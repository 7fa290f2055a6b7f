// What the group-indexed site kernels share (gather_site.hip: mi_gather_site, gather_linear_site.hip:
// mi_gather_linear and mi_gather_slopes): the lane's accumulators, the Poisson rows' constants, what
// a particle and what a (group, particle) fix of a density, the launch's workspace layout and the
// finishing launches (k_gather_sums, k_gather_tables, defined in gather_site.hip and launched
// through gs_finish).
#pragma once
#include "common.hpp"
#include "internal.hpp"

namespace mi {

constexpr int kGsThreads = 256;
constexpr int kGsWaves = kGsThreads / kWave;
constexpr int kGsRows = MI_GATHER_ROWS;
constexpr int kGsBatch = 8;
constexpr int kGsMaxSums = 7;   // the value, two PARTICLE roles, two shifts, two mults

// A sum of float terms: a float over a batch of rows, folded into a double.
struct GsAcc {
  double hi = 0.0;
  float lo = 0.0f;
  __device__ __forceinline__ void add(float x) { lo += x; }
  __device__ __forceinline__ void fold() {
    hi += (double)lo;
    lo = 0.0f;
  }
  __device__ __forceinline__ double take() {
    const double v = hi + (double)lo;
    hi = 0.0;
    lo = 0.0f;
    return v;
  }
};

// Where the launch's partial results go (device pointers into the workspace, and the outputs).
struct GsWork {
  float* sums;          // [nsum][nchunk][K]
  float* slab;          // [2 roles][2 ends][nchunk][K]
  double* rowc;         // [nchunk]: Poisson, the chunk's sum of -lgamma(y + 1)
  int64_t nchunk;
  int nsum;
  int slot_role[2];     // the sum slot of a PARTICLE role, shift, mult; -1: none
  int slot_shift[2];
  int slot_mult[2];
  float* dtable[2];     // GATHER roles' outputs (NULL: not wanted)
  float* out[kGsMaxSums];   // sum slot -> its [K] output (slot 0: total; NULL: not wanted)
};

__device__ __forceinline__ bool gs_non_finite(float x) { return !(fabsf(x) < __builtin_inff()); }

__device__ __forceinline__ float gs_value(const mi_gather_site& L, int64_t row) {
  if (L.value_kind == MI_GATHER_VALUE_INT64)
    return (float)static_cast<const int64_t*>(L.value)[row * L.value_stride_i];
  return static_cast<const float*>(L.value)[row * L.value_stride_i];
}

// Poisson: the sum of -lgamma(y + 1) over the observed rows of the chunk's sorted rows [j0, j1), to
// W.rowc[chunk]. It does not depend on the particle: the first particle tile calls this, its KT
// lanes (kk of them this one) take every KT-th row and meet in a __shfl_xor butterfly.
__device__ __forceinline__ void gs_poisson_rowc(const mi_gather_site& L, const GsWork& W,
                                                int64_t chunk, bool cin, int64_t j0, int64_t j1,
                                                int kk, int KT) {
  double c = 0.0;
  for (int64_t j = j0 + kk; j < j1; j += KT) {
    const int64_t o = L.order[j];
    const int64_t g = L.sorted_group[j];
    if (o < 0 || o >= L.N || g < 0 || g >= L.G) continue;
    if (L.mask != nullptr && L.mask[o * L.mask_stride_i] == 0) continue;
    const float v = gs_value(L, o);
    if (v >= 0.0f) c -= (double)lgammaf(v + 1.0f);
  }
  for (int offset = KT >> 1; offset > 0; offset >>= 1) c += __shfl_xor(c, offset, kWave);
  if (cin && kk == 0) W.rowc[chunk] = c;
}

// The affine terms of a role's predictor eta = shift + mult * p for particle k.
__device__ __forceinline__ float gs_shift(const mi_gather_role& R, int64_t k) {
  return R.shift_kind == MI_GATHER_TERM_PARTICLE ? R.shift[k * R.shift_stride_k]
         : R.shift_kind == MI_GATHER_TERM_CONSTANT ? R.shift_constant : 0.0f;
}

__device__ __forceinline__ float gs_mult(const mi_gather_role& R, int64_t k) {
  return R.mult_kind == MI_GATHER_TERM_PARTICLE ? R.mult[k * R.mult_stride_k]
         : R.mult_kind == MI_GATHER_TERM_CONSTANT ? R.mult_constant : 1.0f;
}

// What particle k fixes of a role: its kind (GATHER, DATA), the affine terms of a GATHER role's
// predictor, and the value of a PARTICLE or CONSTANT role.
__device__ __forceinline__ void gs_role_terms(const mi_gather_role& R, int64_t k, float& shift,
                                              float& mult, float& fixed, bool& gathered,
                                              bool& rowdata) {
  gathered = R.kind == MI_GATHER_GATHER;
  rowdata = R.kind == MI_GATHER_DATA;
  shift = gs_shift(R, k);
  mult = gs_mult(R, k);
  fixed = R.kind == MI_GATHER_PARTICLE ? R.data[k * R.stride_k] : R.constant;
}

// What a (group, particle) fixes of the density, and the row's step.
template <int FAMILY>
struct GsTerms {
  float a0, a1;        // the roles after their links
  float eta0;          // Poisson: log rate
  float c0, c1, c2;    // per-family invariants
  bool bad;            // MI_FLAG_PARAM on an observed row

  __device__ __forceinline__ void derive(bool bad_eta) {
    if constexpr (FAMILY == MI_NORMAL) {
      const float inv = rcp(a1);
      c0 = inv;
      c1 = inv * inv;
      c2 = -(logf(a1) + kHalfLog2Pi);
      bad = bad_eta || !(a1 > 0.0f) || (a0 != a0);
    } else if constexpr (FAMILY == MI_BERNOULLI_LOGITS) {
      const float t = fast_exp(-fabsf(a0));
      const float u = 1.0f + t;
      const float r = rcp(u);
      c0 = fmaxf(a0, 0.0f) + log1p_unit(t, u, r);   // softplus(l)
      c1 = a0 >= 0.0f ? r : t * r;                  // sigmoid(l)
      c2 = 0.0f;
      bad = bad_eta || (a0 != a0);
    } else {
      c0 = c1 = c2 = 0.0f;
      bad = bad_eta;
    }
  }

  // log p and d log p / d role0, d log p / d role1 of a row with value v (Poisson: d / d eta)
  __device__ __forceinline__ void row(float v, float& lp, float& d0, float& d1) const {
    if constexpr (FAMILY == MI_NORMAL) {
      const float diff = v - a0;
      lp = fmaf((-0.5f * c1) * diff, diff, c2);
      const float g = diff * c1;
      d0 = g;
      d1 = fmaf(diff, g, -1.0f) * c0;
    } else if constexpr (FAMILY == MI_BERNOULLI_LOGITS) {
      lp = fmaf(a0, v, -c0);
      d0 = v - c1;
      d1 = 0.0f;
    } else {
      lp = fmaf(v, eta0, -a0);
      d0 = v - a0;
      d1 = 0.0f;
    }
  }

  __device__ __forceinline__ static bool unsupported(float v) {
    if constexpr (FAMILY == MI_NORMAL) return v != v;
    else if constexpr (FAMILY == MI_BERNOULLI_LOGITS) return !(v == 0.0f || v == 1.0f);
    else return !(v >= 0.0f && v == floorf(v));
  }
};

// [lo, hi): the sorted rows of group g (two binary searches of sorted_group [N]).
__device__ __forceinline__ void gs_group_rows(const int32_t* __restrict__ sg, int64_t N, int64_t g,
                                              int64_t& lo, int64_t& hi) {
  int64_t a = 0, b = N;
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if ((int64_t)sg[m] < g) a = m + 1;
    else b = m;
  }
  lo = a;
  b = N;
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if ((int64_t)sg[m] <= g) a = m + 1;
    else b = m;
  }
  hi = a;
}

// ---- host side ------------------------------------------------------------------------------------

inline bool gs_valid_role(const mi_gather_role& R) {
  if (R.kind < MI_GATHER_CONSTANT || R.kind > MI_GATHER_DATA) return false;
  if (R.kind != MI_GATHER_CONSTANT && R.data == nullptr) return false;
  if (R.link != MI_GATHER_LINK_IDENTITY && R.link != MI_GATHER_LINK_EXP) return false;
  if (R.shift_kind < MI_GATHER_TERM_NONE || R.shift_kind > MI_GATHER_TERM_CONSTANT) return false;
  if (R.mult_kind < MI_GATHER_TERM_NONE || R.mult_kind > MI_GATHER_TERM_CONSTANT) return false;
  if (R.shift_kind == MI_GATHER_TERM_PARTICLE && R.shift == nullptr) return false;
  if (R.mult_kind == MI_GATHER_TERM_PARTICLE && R.mult == nullptr) return false;
  return true;
}

inline bool gs_valid(const mi_gather_site* L) {
  return L != nullptr && L->K >= 1 && L->N >= 1 && L->G >= 1 &&
         (L->family == MI_NORMAL || L->family == MI_BERNOULLI_LOGITS || L->family == MI_POISSON) &&
         gs_valid_role(L->role[0]) && gs_valid_role(L->role[1]) &&
         (L->role[0].kind == MI_GATHER_GATHER || L->role[1].kind == MI_GATHER_GATHER) &&
         L->order != nullptr && L->sorted_group != nullptr && L->value != nullptr &&
         (L->value_kind == MI_GATHER_VALUE_FLOAT32 || L->value_kind == MI_GATHER_VALUE_INT64);
}

// The sum slots a site has (whatever gradients a call asks for) and the workspace's parts.
struct GsLayout {
  int64_t nchunk;
  int nsum;
  int slot_role[2], slot_shift[2], slot_mult[2];
  size_t sums_bytes, slab_bytes, rowc_bytes;
  size_t bytes() const { return sums_bytes + slab_bytes + rowc_bytes; }
};

inline size_t gs_round256(size_t n) { return (n + 255) / 256 * 256; }

inline GsLayout gs_layout(const mi_gather_site* L) {
  GsLayout y{};
  y.nchunk = ceil_div(L->N, kGsRows);
  y.nsum = 1;
  for (int r = 0; r < 2; ++r) {
    const mi_gather_role& R = L->role[r];
    const bool gather = R.kind == MI_GATHER_GATHER;
    y.slot_role[r] = R.kind == MI_GATHER_PARTICLE ? y.nsum++ : -1;
    y.slot_shift[r] = gather && R.shift_kind == MI_GATHER_TERM_PARTICLE ? y.nsum++ : -1;
    y.slot_mult[r] = gather && R.mult_kind == MI_GATHER_TERM_PARTICLE ? y.nsum++ : -1;
  }
  const size_t plane = (size_t)y.nchunk * (size_t)L->K * sizeof(float);
  y.sums_bytes = gs_round256(plane * (size_t)y.nsum);
  y.slab_bytes = gs_round256(plane * 4);
  y.rowc_bytes = gs_round256((size_t)y.nchunk * sizeof(double));
  return y;
}

// The site kernel's grid: ktl = log2 of the particle tile, x over blocks of chunks, y over tiles.
struct GsGrid {
  int ktl;
  int64_t gx, gy;
};

inline GsGrid gs_grid(const mi_gather_site* L, const GsLayout& y) {
  GsGrid g{};
  while (g.ktl < 6 && (1 << g.ktl) < L->K) ++g.ktl;
  g.gy = ceil_div(L->K, (int64_t)1 << g.ktl);
  g.gx = ceil_div(y.nchunk, (int64_t)kGsWaves * (kWave >> g.ktl));
  return g;
}

// MI_EUNSUPPORTED conditions of a valid site: a Poisson rate that is not exp of a gathered
// predictor, grids outside the launch limits.
inline bool gs_supported(const mi_gather_site* L, const GsGrid& g) {
  if (L->family == MI_POISSON &&
      !(L->role[0].kind == MI_GATHER_GATHER && L->role[0].link == MI_GATHER_LINK_EXP))
    return false;
  return !(g.gx > kMaxGrid || g.gy > 65535 || L->K > 65535 || ceil_div(L->G, 256) > kMaxGrid ||
           L->N > 0x7FFFFFFF);
}

// The workspace's parts and the outputs of a call, as the kernels take them; table_roles[0..n):
// the GATHER roles whose dtable is wanted (the return value n).
inline int gs_bind(const mi_gather_site* site, const GsLayout& y, void* workspace, float* total,
                   const mi_gather_grads* grads, GsWork& W, int table_roles[2]) {
  char* base = static_cast<char*>(workspace);
  W.sums = reinterpret_cast<float*>(base);
  W.slab = reinterpret_cast<float*>(base + y.sums_bytes);
  W.rowc = reinterpret_cast<double*>(base + y.sums_bytes + y.slab_bytes);
  W.nchunk = y.nchunk;
  W.nsum = y.nsum;
  W.out[0] = total;
  int ntables = 0;
  table_roles[0] = table_roles[1] = 0;
  for (int r = 0; r < 2; ++r) {
    W.slot_role[r] = y.slot_role[r];
    W.slot_shift[r] = y.slot_shift[r];
    W.slot_mult[r] = y.slot_mult[r];
    const bool gather = site->role[r].kind == MI_GATHER_GATHER;
    // (a Bernoulli or Poisson site has no second role: nothing of it is written)
    const bool live = r == 0 || site->family == MI_NORMAL;
    float* out = grads != nullptr && live ? grads->role[r] : nullptr;
    W.dtable[r] = gather ? out : nullptr;
    if (W.dtable[r] != nullptr) table_roles[ntables++] = r;
    if (y.slot_role[r] >= 0) W.out[y.slot_role[r]] = out;
    if (y.slot_shift[r] >= 0) W.out[y.slot_shift[r]] = grads != nullptr && live ? grads->shift[r] : nullptr;
    if (y.slot_mult[r] >= 0) W.out[y.slot_mult[r]] = grads != nullptr && live ? grads->mult[r] : nullptr;
  }
  return ntables;
}

// The finishing launches of a call (gather_site.hip): the chunks' sums in chunk order, then the
// dtable entries the site kernel did not store itself. 0 or an MI_* code.
int gs_finish(const mi_gather_site* site, const GsWork& W, double gscale, const int table_roles[2],
              int ntables, hipStream_t s);

// The launch that finishes dtheta (gather_linear_site.hip, k_gather_dtheta): dtheta[k, j] =
// gscale * the sum over the chunks of dth[j][chunk][k], in chunk order. 0 or an MI_* code.
int gl_dtheta(const float* dth, int64_t nchunk, int64_t K, int P, double gscale, float* dtheta,
              hipStream_t s);

}  // namespace mi
