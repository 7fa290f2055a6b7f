// Group-indexed sites with a linear predictor: Normal / Bernoulli-logits / Poisson over N rows whose
// first parameter is the multilevel regression's predictor
//   eta0[k, i] = shift_k + mult_k * alpha[k, g_i] + sum_{s < S} beta_s[k, g_i] * z_s[i]
//              + sum_{j < P} X[i, j] * theta[k, j]
// (include/mininf_amd.h: mi_gather_linear is S = 0 and P >= 1, mi_gather_slopes S >= 1 and P >= 0).
// The layout is gather_site.hip's: a lane owns one particle and walks the kGsRows consecutive sorted
// rows of its chunk, a group's sum of d log p / d eta0 stays in the lane and is stored to dtable when
// the group ends, neighbours' parts go through the slab, k_gather_sums and k_gather_tables finish in
// chunk order. What differs:
//   - eta0 changes with every row, so nothing of role 0 is hoisted to the group: an observed row
//     derives the density's terms itself (the path k_gather_site has for DATA roles). What a group
//     fixes of role 1 (a Normal's 1 / sigma^2 and log sigma) is still evaluated once per group;
//   - eta0 is built in a fixed order: fmaf(mult, alpha, shift), then one fmaf(beta_s, z_s, eta) per
//     slope s = 0..S-1, then one fmaf(X[i, j], theta[j], eta) per column j = 0..P-1;
//   - the lane holds theta[k, 0..P) and the P sums of dtheta in registers: a float over a batch of
//     kGsBatch rows, folded into a float over the chunk (8 + 32 roundings of a sum, against the
//     256 of a plain float sum);
//   - every lane of a particle tile reads the row of X at one address (float4 loads where X's rows
//     are contiguous and 16-byte aligned). A masked-out row reads nothing of X;
//   - the chunk's P sums leave the lane once, into the slab dth[P][chunks][K] (consecutive lanes,
//     consecutive addresses); k_gather_dtheta adds the chunks in ascending order in fp64;
//   - on a group change the lane also loads beta_s[k, g], s < S: S loads strided by G across the
//     lanes, like the intercept's table entry;
//   - an observed row reads z_s[o] at one address per particle tile, issued with the batch's other
//     row loads (value, mask, a DATA role); a masked-out row reads no z;
//   - de * z_s is summed per slope the way seg[0] sums de: fmaf into a float over the batch of
//     kGsBatch rows, folded into a double that lasts the group;
//   - at the group's end the sum goes to dslope_s[k, g], or to the slope slab
//     [S][2 ends][chunks][K] when the group continues in a neighbouring chunk;
//     k_gather_slope_tables (k_gather_tables' sibling) writes the zeros of the empty groups and adds
//     the parts of a group that spans chunks: its tail, then the heads in ascending chunk order, fp64.
// Instantiated by P bucket (0, 8, 16, 32) and S bucket (0, 1, 2, 4) so that a small site does not pay
// for the registers of a large one: P = 0 holds nothing of X or theta, S = 0 nothing of a slope.
// (0, 0) is k_gather_site's and has no instance.
// No atomics, and every sum has a fixed order: two launches give the same bits.
#include "gather_common.hpp"

#include <cstdint>

namespace mi {

// Where the slope sums go (device pointers).
struct GsSlopeWork {
  float* slab;                            // [S][2 ends][nchunk][K]
  float* dslope[MI_GATHER_MAX_SLOPES];    // [K, G] contiguous, or NULL: not wanted
};

// Grid: x over blocks of kGsWaves * (64 >> ktl) chunks, y over tiles of 1 << ktl particles.
template <int FAMILY, int PB, int SB>
__global__ __launch_bounds__(kGsThreads) void k_gather_linear(const mi_gather_slopes M, const GsWork W,
                                                              const GsSlopeWork V,
                                                              float* __restrict__ dth, int ktl,
                                                              double gscale,
                                                              uint32_t* __restrict__ flags) {
  static_assert(PB > 0 || SB > 0, "a site with neither columns nor slopes is k_gather_site's");
  constexpr int PA = PB > 0 ? PB : 1;   // (arrays of a P = 0 or S = 0 instance: one dead element)
  constexpr int SA = SB > 0 ? SB : 1;
  const mi_gather_linear& LL = M.linear;
  const mi_gather_site& L = LL.site;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int KT = 1 << ktl;
  const int sub = lane >> ktl, kk = lane & (KT - 1);
  const int64_t K = L.K, N = L.N, G = L.G;
  const int P = (int)LL.P, S = (int)M.S;
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
  if (FAMILY == MI_POISSON && blockIdx.y == 0) gs_poisson_rowc(L, W, chunk, cin, j0, j1, kk, KT);

  // ---- what the particle fixes -------------------------------------------------------------------
  float shift[2], mult[2], praw[2] = {0.0f, 0.0f}, fixed[2];
  bool gathered[2], rowdata[2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
    gs_role_terms(L.role[r], k, shift[r], mult[r], fixed[r], gathered[r], rowdata[r]);
  float th[PA], lo[PA], hi[PA];
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
  float beta[SA];        // beta_s[k, g] of the current group
#pragma unroll
  for (int s = 0; s < SB; ++s) beta[s] = 0.0f;
  float chain1 = 1.0f;   // d role 1 / d eta of a GATHER role
  bool bad1 = false;     // what role 1 adds to MI_FLAG_PARAM
  GsAcc seg[2], sacc[SA], lpacc, rolacc;
  double dshift[2] = {0.0, 0.0}, dmult[2] = {0.0, 0.0};
  int gcur = 0;
  bool started = false, gvalid = false;
  int nseg = 0;

  // the group that just ended: its sums to dtable and dslope (or the slabs), to d shift and d mult
  auto flush = [&](bool last) {
    const bool to_head = nseg == 0 && head_shared;
    const bool to_tail = last && tail_shared && !to_head;
    const bool store = gvalid && kin;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!gathered[r]) continue;
      const double Sr = seg[r].take();
      dshift[r] += Sr;
      if (Sr != 0.0) dmult[r] += (double)praw[r] * Sr;   // (a group of masked rows: whatever p holds)
      if (!store || W.dtable[r] == nullptr) continue;
      if (to_head || to_tail)
        W.slab[(((int64_t)r * 2 + (to_head ? 0 : 1)) * W.nchunk + chunk) * K + k] = (float)Sr;
      else
        W.dtable[r][k * G + gcur] = (float)(gscale * (double)mult[r] * Sr);
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const double Ss = sacc[s].take();
      if (s >= S || !store || V.dslope[s] == nullptr) continue;
      if (to_head || to_tail)
        V.slab[(((int64_t)s * 2 + (to_head ? 0 : 1)) * W.nchunk + chunk) * K + k] = (float)Ss;
      else
        V.dslope[s][k * G + gcur] = (float)(gscale * Ss);
    }
    ++nseg;
  };

  for (int64_t jb = j0; jb < j1; jb += kGsBatch) {
    int gi[kGsBatch];
    int64_t oi[kGsBatch];
    float vv[kGsBatch], d1v[kGsBatch], zv[SA][kGsBatch];
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
#pragma unroll
      for (int s = 0; s < SB; ++s)
        zv[s][u] = (s < S && ob[u]) ? M.slope[s].z[o * M.slope[s].z_stride_i] : 0.0f;
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
#pragma unroll
        for (int s = 0; s < SB; ++s)
          beta[s] = (s < S && gvalid)
                        ? M.slope[s].table[k * M.slope[s].stride_k + (int64_t)g * M.slope[s].stride_g]
                        : 0.0f;
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
      float xr[PA];
      if constexpr (PB > 0) {
        const float* __restrict__ const xrow = X + oi[u] * sxi;
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
      }
      // intercept base, then the slopes 0..S-1, then the columns of X
      float eta = base0;
#pragma unroll
      for (int s = 0; s < SB; ++s)
        if (s < S) eta = fmaf(beta[s], zv[s][u], eta);
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
      for (int s = 0; s < SB; ++s) sacc[s].lo = fmaf(de, zv[s][u], sacc[s].lo);
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
    for (int s = 0; s < SB; ++s) sacc[s].fold();
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
    if (PB > 0 && dth != nullptr) {
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

// dslope_s[k, g] of the groups the site kernel did not store itself: 0 for a group without rows,
// the slope slab's parts in chunk order (fp64) for a group whose rows span chunks. Grid: x over
// groups, y over particles, z over the slopes (one without a dslope returns at once).
__global__ __launch_bounds__(256) void k_gather_slope_tables(const int32_t* __restrict__ sg, int64_t N,
                                                             int64_t G, int64_t K, int64_t nchunk,
                                                             const GsSlopeWork V, double gscale) {
  const int s = blockIdx.z;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (g >= G || V.dslope[s] == nullptr) return;
  int64_t lo, hi;
  gs_group_rows(sg, N, g, lo, hi);
  float* const dst = V.dslope[s] + k * G + g;
  if (lo == hi) {
    *dst = 0.0f;
    return;
  }
  const int64_t c0 = lo / kGsRows, c1 = (hi - 1) / kGsRows;
  if (c0 == c1) return;   // stored by the chunk that holds all its rows
  // the chunk where the group starts left its tail, every later one its head
  double sum = (double)V.slab[(((int64_t)s * 2 + 1) * nchunk + c0) * K + k];
  for (int64_t c = c0 + 1; c <= c1; ++c) sum += (double)V.slab[(((int64_t)s * 2) * nchunk + c) * K + k];
  *dst = (float)(gscale * sum);
}

}  // namespace mi

namespace {

// MI_EINVAL conditions of the two entry points; S > MI_GATHER_MAX_SLOPES and
// P > MI_GATHER_LINEAR_MAX_P are unsupported
bool valid(const mi_gather_linear* L) {
  return L != nullptr && mi::gs_valid(&L->site) && L->site.role[0].kind == MI_GATHER_GATHER &&
         L->P >= 1 && L->x != nullptr && L->theta != nullptr;
}

bool valid(const mi_gather_slopes* M) {
  if (M == nullptr) return false;
  const mi_gather_linear& L = M->linear;
  if (!mi::gs_valid(&L.site) || L.site.role[0].kind != MI_GATHER_GATHER) return false;
  if (L.P < 0 || (L.P >= 1 && (L.x == nullptr || L.theta == nullptr))) return false;
  if (M->S < 1) return false;
  for (int64_t s = 0; s < M->S && s < MI_GATHER_MAX_SLOPES; ++s)
    if (M->slope[s].table == nullptr || M->slope[s].z == nullptr) return false;
  return true;
}

bool too_large(const mi_gather_slopes* M) {
  return M->S > MI_GATHER_MAX_SLOPES || M->linear.P > MI_GATHER_LINEAR_MAX_P;
}

// a valid mi_gather_linear as the site without slopes that the kernel takes
mi_gather_slopes without_slopes(const mi_gather_linear* L) {
  mi_gather_slopes M{};
  M.linear = *L;
  return M;
}

// the workspace: mi_gather_site's, the dtheta slab [P][chunks][K], the slope slab
struct Parts {
  size_t site, dtheta, slopes;
  size_t bytes() const { return site + dtheta + slopes; }
};

Parts parts_of(const mi_gather_slopes* M, const mi::GsLayout& y) {
  const size_t plane = (size_t)y.nchunk * (size_t)M->linear.site.K * sizeof(float);
  return Parts{y.bytes(), mi::gs_round256(plane * (size_t)M->linear.P),
               mi::gs_round256(plane * 2 * (size_t)M->S)};
}

int workspace_bytes(const mi_gather_slopes* M, size_t* bytes) {
  if (too_large(M)) return MI_EUNSUPPORTED;
  *bytes = parts_of(M, mi::gs_layout(&M->linear.site)).bytes();
  return 0;
}

struct Launch {
  const mi_gather_slopes* M;
  mi::GsWork W;
  mi::GsSlopeWork V;
  float* dth;
  mi::GsGrid g;
  double gscale;
  uint32_t* flags;
  hipStream_t s;
};

template <int FAMILY, int PB, int SB>
void launch(const Launch& a) {
  hipLaunchKernelGGL((mi::k_gather_linear<FAMILY, PB, SB>), dim3((unsigned)a.g.gx, (unsigned)a.g.gy),
                     dim3(mi::kGsThreads), 0, a.s, *a.M, a.W, a.V, a.dth, a.g.ktl, a.gscale, a.flags);
}

template <int FAMILY, int PB>
void launch_slopes(const Launch& a) {
  const int64_t S = a.M->S;
  if constexpr (PB > 0) {   // (neither entry point lets P = 0 with S = 0 pass)
    if (S == 0) return launch<FAMILY, PB, 0>(a);
  }
  if (S <= 1) launch<FAMILY, PB, 1>(a);
  else if (S <= 2) launch<FAMILY, PB, 2>(a);
  else launch<FAMILY, PB, 4>(a);
}

template <int FAMILY>
void launch_bucket(const Launch& a) {
  const int64_t P = a.M->linear.P;
  if (P == 0) launch_slopes<FAMILY, 0>(a);
  else if (P <= 8) launch_slopes<FAMILY, 8>(a);
  else if (P <= 16) launch_slopes<FAMILY, 16>(a);
  else launch_slopes<FAMILY, 32>(a);
}

// The call of either entry point on a site that passed its valid(): S may be 0.
int forward(const mi_gather_slopes* site, void* workspace, size_t workspace_bytes, float* total,
            const mi_gather_grads* grads, float* dtheta, float* const* dslope, uint32_t* flags,
            void* stream) {
  const mi_gather_site* base = &site->linear.site;
  const mi::GsLayout y = mi::gs_layout(base);
  Launch a{};
  a.M = site;
  a.g = mi::gs_grid(base, y);
  if (too_large(site) || !mi::gs_supported(base, a.g)) return MI_EUNSUPPORTED;
  const Parts parts = parts_of(site, y);
  if (workspace == nullptr || workspace_bytes < parts.bytes()) return MI_EWORKSPACE;
  a.s = static_cast<hipStream_t>(stream);
  a.flags = flags;
  hipError_t e;
  if (!(base->options & MI_GROUP_FLAGS_ZEROED)) {
    if ((e = hipMemsetAsync(flags, 0, sizeof(uint32_t), a.s)) != hipSuccess) return to_code(e);
  }
  int table_roles[2];
  const int ntables = mi::gs_bind(base, y, workspace, total, grads, a.W, table_roles);
  const int64_t P = site->linear.P;
  a.dth = dtheta != nullptr && P > 0
              ? reinterpret_cast<float*>(static_cast<char*>(workspace) + parts.site)
              : nullptr;
  a.V.slab = reinterpret_cast<float*>(static_cast<char*>(workspace) + parts.site + parts.dtheta);
  bool any_slope = false;
  for (int64_t q = 0; q < site->S; ++q) {
    a.V.dslope[q] = dslope != nullptr ? dslope[q] : nullptr;
    any_slope = any_slope || a.V.dslope[q] != nullptr;
  }
  a.gscale = (double)base->grad_scale * base->site_scale;
  if (base->family == MI_NORMAL) launch_bucket<MI_NORMAL>(a);
  else if (base->family == MI_BERNOULLI_LOGITS) launch_bucket<MI_BERNOULLI_LOGITS>(a);
  else launch_bucket<MI_POISSON>(a);
  if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  int code = mi::gs_finish(base, a.W, a.gscale, table_roles, ntables, a.s);
  if (code != 0) return code;
  if (any_slope) {
    hipLaunchKernelGGL(mi::k_gather_slope_tables,
                       dim3((unsigned)ceil_div(base->G, 256), (unsigned)base->K, (unsigned)site->S),
                       dim3(256), 0, a.s, base->sorted_group, base->N, base->G, base->K, y.nchunk, a.V,
                       a.gscale);
    if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  }
  if (a.dth != nullptr) return mi::gl_dtheta(a.dth, y.nchunk, base->K, (int)P, a.gscale, dtheta, a.s);
  return 0;
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
  const mi_gather_slopes M = without_slopes(site);
  return workspace_bytes(&M, bytes);
}

int mi_gather_linear_forward(const mi_gather_linear* site, void* workspace, size_t workspace_bytes,
                             float* total, const mi_gather_grads* grads, float* dtheta,
                             uint32_t* flags, void* stream) {
  if (!valid(site) || total == nullptr || flags == nullptr) return MI_EINVAL;
  const mi_gather_slopes M = without_slopes(site);
  return forward(&M, workspace, workspace_bytes, total, grads, dtheta, nullptr, flags, stream);
}

int mi_gather_slopes_struct_size(size_t* bytes) {
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = sizeof(mi_gather_slopes);
  return 0;
}

int mi_gather_slopes_workspace_bytes(const mi_gather_slopes* site, size_t* bytes) {
  if (!valid(site) || bytes == nullptr) return MI_EINVAL;
  return workspace_bytes(site, bytes);
}

int mi_gather_slopes_forward(const mi_gather_slopes* site, void* workspace, size_t workspace_bytes,
                             float* total, const mi_gather_grads* grads, float* dtheta,
                             float* const dslope[MI_GATHER_MAX_SLOPES], uint32_t* flags,
                             void* stream) {
  if (!valid(site) || total == nullptr || flags == nullptr) return MI_EINVAL;
  return forward(site, workspace, workspace_bytes, total, grads, dtheta, dslope, flags, stream);
}

}  // extern "C"
