// Group-indexed sites with fixed effects: Normal / Bernoulli-logits / Poisson over N rows whose
// first parameter is the multilevel regression's predictor
//   eta0[k, i] = shift_k + mult_k * table[k, group_i] + sum_j X[i, j] * theta[k, j]
// (include/mininf_amd.h, mi_gather_linear). The layout is gather_site.hip's: a lane owns one
// particle and walks the kGsRows consecutive sorted rows of its chunk, a group's sum of
// d log p / d eta0 stays in the lane and is stored to dtable when the group ends, neighbours' parts
// go through the slab, k_gather_sums and k_gather_tables finish in chunk order. What differs:
//   - eta0 changes with every row, so nothing of role 0 is hoisted to the group: an observed row
//     derives the density's terms itself (the path k_gather_site has for DATA roles). What a group
//     fixes of role 1 (a Normal's 1 / sigma^2 and log sigma) is still evaluated once per group;
//   - the lane holds theta[k, 0..P) and the P sums of dtheta in registers: a float over a batch of
//     kGsBatch rows, folded into a float over the chunk (8 + 32 roundings of a sum, against the
//     256 of a plain float sum). The kernel is instantiated by P bucket (8, 16, 32) so that a
//     small P does not pay for the registers of a large one;
//   - every lane of a particle tile reads the row of X at one address (float4 loads where X's rows
//     are contiguous and 16-byte aligned). A masked-out row reads nothing of X;
//   - the chunk's P sums leave the lane once, into the slab dth[P][chunks][K] (consecutive lanes,
//     consecutive addresses); k_gather_dtheta adds the chunks in ascending order in fp64.
// No atomics, and every sum has a fixed order: two launches give the same bits.
#include "gather_common.hpp"

#include <cstdint>

namespace mi {

// Grid: x over blocks of kGsWaves * (64 >> ktl) chunks, y over tiles of 1 << ktl particles.
template <int FAMILY, int PB>
__global__ __launch_bounds__(kGsThreads) void k_gather_linear(const mi_gather_linear LL, const GsWork W,
                                                              float* __restrict__ dth, int ktl,
                                                              double gscale,
                                                              uint32_t* __restrict__ flags) {
  const mi_gather_site& L = LL.site;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int KT = 1 << ktl;
  const int sub = lane >> ktl, kk = lane & (KT - 1);
  const int64_t K = L.K, N = L.N, G = L.G;
  const int P = (int)LL.P;
  const int64_t chunk = ((int64_t)blockIdx.x * kGsWaves + wave) * (kWave >> ktl) + sub;
  const int64_t kreal = (int64_t)blockIdx.y * KT + kk;
  const bool kin = kreal < K;
  const int64_t k = kin ? kreal : K - 1;   // lanes past K repeat the last particle and store nothing
  const bool cin = chunk < W.nchunk;
  const int64_t j0 = cin ? chunk * kGsRows : 0;
  const int64_t j1 = cin ? min(N, j0 + kGsRows) : 0;
  const int32_t* __restrict__ const sg = L.sorted_group;
  const int32_t* __restrict__ const ord = L.order;
  uint32_t fl = 0u;

  // ---- Poisson: the chunk's sum of -lgamma(y + 1) over its observed rows, by the first tile ------
  if (FAMILY == MI_POISSON && blockIdx.y == 0) {
    double c = 0.0;
    for (int64_t j = j0 + kk; j < j1; j += KT) {
      const int64_t o = ord[j];
      const int64_t g = sg[j];
      if (o < 0 || o >= N || g < 0 || g >= G) continue;
      if (L.mask != nullptr && L.mask[o * L.mask_stride_i] == 0) continue;
      const float v = gs_value(L, o);
      if (v >= 0.0f) c -= (double)lgammaf(v + 1.0f);
    }
    for (int offset = KT >> 1; offset > 0; offset >>= 1) c += __shfl_xor(c, offset, kWave);
    if (cin && kk == 0) W.rowc[chunk] = c;
  }

  // ---- what the particle fixes -------------------------------------------------------------------
  float shift[2], mult[2], praw[2] = {0.0f, 0.0f}, fixed[2];
  bool gathered[2], rowdata[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const mi_gather_role& R = L.role[r];
    gathered[r] = R.kind == MI_GATHER_GATHER;
    rowdata[r] = R.kind == MI_GATHER_DATA;
    shift[r] = R.shift_kind == MI_GATHER_TERM_PARTICLE ? R.shift[k * R.shift_stride_k]
               : R.shift_kind == MI_GATHER_TERM_CONSTANT ? R.shift_constant : 0.0f;
    mult[r] = R.mult_kind == MI_GATHER_TERM_PARTICLE ? R.mult[k * R.mult_stride_k]
              : R.mult_kind == MI_GATHER_TERM_CONSTANT ? R.mult_constant : 1.0f;
    fixed[r] = R.kind == MI_GATHER_PARTICLE ? R.data[k * R.stride_k] : R.constant;
  }
  float th[PB], lo[PB], hi[PB];
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    th[j] = j < P ? LL.theta[k * LL.theta_stride_k + j * LL.theta_stride_j] : 0.0f;
    lo[j] = hi[j] = 0.0f;
  }
  const float* __restrict__ const X = LL.x;
  const int64_t sxi = LL.x_stride_i, sxj = LL.x_stride_j;
  // rows of X that float4 loads can read: contiguous, and every row 16-byte aligned
  const bool vec = sxj == 1 && (sxi & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const bool exp0 = L.role[0].link == MI_GATHER_LINK_EXP;
  const bool head_shared = cin && j0 > 0 && sg[j0 - 1] == sg[j0];
  const bool tail_shared = cin && j1 < N && sg[j1] == sg[j1 - 1];

  GsTerms<FAMILY> T;
  T.a0 = 0.0f;
  T.a1 = fixed[1];
  T.eta0 = 0.0f;
  T.c0 = T.c1 = T.c2 = 0.0f;
  T.bad = false;
  float base0 = 0.0f;    // shift + mult * table[k, g] of role 0
  float chain1 = 1.0f;   // d role 1 / d eta of a GATHER role
  bool bad1 = false;     // what role 1 adds to MI_FLAG_PARAM
  GsAcc seg[2], lpacc, rolacc;
  double dshift[2] = {0.0, 0.0}, dmult[2] = {0.0, 0.0};
  int gcur = 0;
  bool started = false, gvalid = false;
  int nseg = 0;

  // the group that just ended: its sums to dtable (or the slab), to d shift and d mult
  auto flush = [&](bool last) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!gathered[r]) continue;
      const double S = seg[r].take();
      dshift[r] += S;
      if (S != 0.0) dmult[r] += (double)praw[r] * S;   // (a group of masked rows: whatever p holds)
      if (!gvalid || W.dtable[r] == nullptr || !kin) continue;
      const bool to_head = nseg == 0 && head_shared;
      const bool to_tail = last && tail_shared && !to_head;
      if (to_head || to_tail)
        W.slab[(((int64_t)r * 2 + (to_head ? 0 : 1)) * W.nchunk + chunk) * K + k] = (float)S;
      else
        W.dtable[r][k * G + gcur] = (float)(gscale * (double)mult[r] * S);
    }
    ++nseg;
  };

  for (int64_t jb = j0; jb < j1; jb += kGsBatch) {
    int gi[kGsBatch];
    int64_t oi[kGsBatch];
    float vv[kGsBatch], d1v[kGsBatch];
    bool ob[kGsBatch];
#pragma unroll
    for (int u = 0; u < kGsBatch; ++u) {
      const int64_t j = min(jb + u, j1 - 1);
      gi[u] = sg[j];
      oi[u] = ord[j];
    }
#pragma unroll
    for (int u = 0; u < kGsBatch; ++u) {
      const bool in = jb + u < j1;
      const bool okrow = oi[u] >= 0 && oi[u] < N;
      const bool okgroup = gi[u] >= 0 && (int64_t)gi[u] < G;
      const int64_t o = okrow ? oi[u] : 0;
      oi[u] = o;
      vv[u] = gs_value(L, o);
      const bool m = L.mask == nullptr || L.mask[o * L.mask_stride_i] != 0;
      d1v[u] = rowdata[1] ? L.role[1].data[o * L.role[1].stride_g] : 0.0f;
      ob[u] = in && okrow && okgroup && m;
      fl |= (in && !(okrow && okgroup)) ? MI_FLAG_INTERNAL : 0u;
    }
#pragma unroll
    for (int u = 0; u < kGsBatch; ++u) {
      if (jb + u >= j1) break;
      const int g = gi[u];
      const bool changed = !started || g != gcur;
      if (changed) {
        if (started) flush(false);
        started = true;
        gcur = g;
        gvalid = g >= 0 && (int64_t)g < G;
        praw[0] = gvalid ? L.role[0].data[k * L.role[0].stride_k + (int64_t)g * L.role[0].stride_g]
                         : 0.0f;
        base0 = fmaf(mult[0], praw[0], shift[0]);
      }
      if (changed || rowdata[1]) {
        float a1 = rowdata[1] ? d1v[u] : fixed[1];
        bool bad_eta1 = false;
        chain1 = 1.0f;
        if (gathered[1]) {
          if (changed)
            praw[1] = gvalid ? L.role[1].data[k * L.role[1].stride_k + (int64_t)g * L.role[1].stride_g]
                             : 0.0f;
          const float eta1 = fmaf(mult[1], praw[1], shift[1]);
          bad_eta1 = gs_non_finite(eta1);
          a1 = eta1;
          if (L.role[1].link == MI_GATHER_LINK_EXP) {
            a1 = fast_exp(eta1);
            if (FAMILY != MI_POISSON) chain1 = a1;
          }
        }
        T.a1 = a1;
        if constexpr (FAMILY == MI_NORMAL) {
          T.derive(false);   // 1 / sigma, 1 / sigma^2, -log sigma - log sqrt(2 pi)
          bad1 = bad_eta1 || !(a1 > 0.0f);
        } else {
          bad1 = bad_eta1;
        }
      }
      if (!ob[u]) continue;
      // ---- the row of X, eta0 and the density's terms ----------------------------------------------
      const float* __restrict__ const xrow = X + oi[u] * sxi;
      float xr[PB];
#pragma unroll
      for (int q = 0; q < PB / 4; ++q) {
        if (vec && 4 * q + 3 < P) {
          const float4 t = *reinterpret_cast<const float4*>(xrow + 4 * q);
          xr[4 * q] = t.x;
          xr[4 * q + 1] = t.y;
          xr[4 * q + 2] = t.z;
          xr[4 * q + 3] = t.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) xr[4 * q + e] = 4 * q + e < P ? xrow[(4 * q + e) * sxj] : 0.0f;
        }
      }
      float eta = base0;
#pragma unroll
      for (int j = 0; j < PB; ++j) eta = fmaf(xr[j], th[j], eta);
      const bool bad_eta = gs_non_finite(eta);
      float a0 = eta, chain0 = 1.0f;
      if (exp0) {
        a0 = fast_exp(eta);
        if (FAMILY != MI_POISSON) chain0 = a0;
      }
      T.a0 = a0;
      T.eta0 = eta;
      if constexpr (FAMILY == MI_NORMAL) T.bad = bad_eta || bad1 || (a0 != a0);
      else T.derive(bad_eta || bad1);
      float lp, d0, d1;
      T.row(vv[u], lp, d0, d1);
      lpacc.add(lp);
      fl |= (T.bad ? MI_FLAG_PARAM : 0u) | (T.unsupported(vv[u]) ? MI_FLAG_SUPPORT : 0u);
      const float de = d0 * chain0;
      seg[0].add(de);
#pragma unroll
      for (int j = 0; j < PB; ++j) lo[j] = fmaf(de, xr[j], lo[j]);
      if (FAMILY == MI_NORMAL) {
        if (gathered[1]) seg[1].add(d1 * chain1);
        else rolacc.add(d1);
      }
    }
    seg[0].fold();
    seg[1].fold();
    lpacc.fold();
    rolacc.fold();
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      hi[j] += lo[j];
      lo[j] = 0.0f;
    }
  }
  if (started) flush(true);

  if (cin && kin) {
    float* const base = W.sums + chunk * K + k;
    const int64_t plane = W.nchunk * K;
    base[0] = (float)lpacc.take();
    if (W.slot_role[1] >= 0) base[W.slot_role[1] * plane] = (float)rolacc.take();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (W.slot_shift[r] >= 0) base[W.slot_shift[r] * plane] = (float)dshift[r];
      if (W.slot_mult[r] >= 0) base[W.slot_mult[r] * plane] = (float)dmult[r];
    }
    if (dth != nullptr) {
      float* const d = dth + chunk * K + k;
#pragma unroll
      for (int j = 0; j < PB; ++j)
        if (j < P) d[j * plane] = hi[j];
    }
  }
  publish_flags(flags, fl);
}

// dtheta[k, j] = gscale * sum_chunks dth[j][chunk][k], chunks ascending (fp64). A block takes 32
// particles of one j; its kGlParts thread rows take every kGlParts-th chunk and meet in LDS, added
// in their order (k_gather_sums' scheme).
constexpr int kGlParts = 32;
__global__ __launch_bounds__(32 * kGlParts) void k_gather_dtheta(const float* __restrict__ dth,
                                                                 int64_t nchunk, int64_t K, int P,
                                                                 double gscale,
                                                                 float* __restrict__ dtheta) {
  __shared__ double red[kGlParts][32];
  const int kq = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int j = blockIdx.y;
  const int64_t k = (int64_t)blockIdx.x * 32 + kq;
  double v = 0.0;
  if (k < K) {
    const float* src = dth + (int64_t)j * nchunk * K + k;
    for (int64_t c = part; c < nchunk; c += kGlParts) v += (double)src[c * K];
  }
  red[part][kq] = v;
  __syncthreads();
  if (part == 0 && k < K) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < kGlParts; ++p) s += red[p][kq];
    dtheta[k * P + j] = (float)(gscale * s);
  }
}

// (gather_common.hpp)
int gl_dtheta(const float* dth, int64_t nchunk, int64_t K, int P, double gscale, float* dtheta,
              hipStream_t s) {
  hipLaunchKernelGGL(k_gather_dtheta, dim3((unsigned)ceil_div(K, 32), (unsigned)P),
                     dim3(32 * kGlParts), 0, s, dth, nchunk, K, P, gscale, dtheta);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? to_code(e) : 0;
}

}  // namespace mi

namespace {

bool valid(const mi_gather_linear* L) {
  return L != nullptr && mi::gs_valid(&L->site) && L->site.role[0].kind == MI_GATHER_GATHER &&
         L->P >= 1 && L->x != nullptr && L->theta != nullptr;
}

size_t dtheta_bytes(const mi_gather_linear* L, const mi::GsLayout& y) {
  return mi::gs_round256((size_t)y.nchunk * (size_t)L->site.K * (size_t)L->P * sizeof(float));
}

template <int FAMILY>
void launch_bucket(const mi_gather_linear* L, const mi::GsWork& W, float* dth, const mi::GsGrid& g,
                   double gscale, uint32_t* flags, hipStream_t s) {
  const dim3 grid((unsigned)g.gx, (unsigned)g.gy), block(mi::kGsThreads);
  if (L->P <= 8)
    hipLaunchKernelGGL((mi::k_gather_linear<FAMILY, 8>), grid, block, 0, s, *L, W, dth, g.ktl, gscale,
                       flags);
  else if (L->P <= 16)
    hipLaunchKernelGGL((mi::k_gather_linear<FAMILY, 16>), grid, block, 0, s, *L, W, dth, g.ktl, gscale,
                       flags);
  else
    hipLaunchKernelGGL((mi::k_gather_linear<FAMILY, 32>), grid, block, 0, s, *L, W, dth, g.ktl, gscale,
                       flags);
}

}  // namespace

extern "C" {

int mi_gather_linear_struct_size(size_t* bytes) {
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = sizeof(mi_gather_linear);
  return 0;
}

int mi_gather_linear_workspace_bytes(const mi_gather_linear* site, size_t* bytes) {
  if (!valid(site) || bytes == nullptr) return MI_EINVAL;
  if (site->P > MI_GATHER_LINEAR_MAX_P) return MI_EUNSUPPORTED;
  const mi::GsLayout y = mi::gs_layout(&site->site);
  *bytes = y.bytes() + dtheta_bytes(site, y);
  return 0;
}

int mi_gather_linear_forward(const mi_gather_linear* site, void* workspace, size_t workspace_bytes,
                             float* total, const mi_gather_grads* grads, float* dtheta,
                             uint32_t* flags, void* stream) {
  if (!valid(site) || total == nullptr || flags == nullptr) return MI_EINVAL;
  const mi_gather_site* base = &site->site;
  const mi::GsLayout y = mi::gs_layout(base);
  const mi::GsGrid g = mi::gs_grid(base, y);
  if (site->P > MI_GATHER_LINEAR_MAX_P || !mi::gs_supported(base, g)) return MI_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < y.bytes() + dtheta_bytes(site, y)) return MI_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (!(base->options & MI_GROUP_FLAGS_ZEROED)) {
    if ((e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s)) != hipSuccess) return to_code(e);
  }
  mi::GsWork W{};
  int table_roles[2];
  const int ntables = mi::gs_bind(base, y, workspace, total, grads, W, table_roles);
  float* const dth = dtheta != nullptr
                         ? reinterpret_cast<float*>(static_cast<char*>(workspace) + y.bytes())
                         : nullptr;
  const double gscale = (double)base->grad_scale * base->site_scale;
  if (base->family == MI_NORMAL) launch_bucket<MI_NORMAL>(site, W, dth, g, gscale, flags, s);
  else if (base->family == MI_BERNOULLI_LOGITS)
    launch_bucket<MI_BERNOULLI_LOGITS>(site, W, dth, g, gscale, flags, s);
  else launch_bucket<MI_POISSON>(site, W, dth, g, gscale, flags, s);
  if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  const int code = mi::gs_finish(base, W, gscale, table_roles, ntables, s);
  if (code != 0) return code;
  if (dtheta != nullptr) return mi::gl_dtheta(dth, y.nchunk, base->K, (int)site->P, gscale, dtheta, s);
  return 0;
}

}  // extern "C"
