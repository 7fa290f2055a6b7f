// Group-indexed sites: Normal / Bernoulli-logits / Poisson over N rows whose parameter is the
// model's own gather table[index] of a per-particle table [K, G] (include/mininf_amd.h,
// mi_gather_site).
//
// Traced over K particles the model's `alpha[group]` is a [K, N] gather that the site kernel reads
// as a dense operand, the site writes a dense [K, N] gradient and torch's index backward scatters
// it into [K, G] with float atomics. Here the rows arrive sorted by group (order, sorted_group), so
// the rows of a group are consecutive and the scatter is a segmented sum:
//   - a lane owns one particle and walks the kGsRows consecutive sorted rows of its chunk; a wave
//     is KT = min(64, next_pow2(K)) particles by 64 / KT chunks, a block four waves;
//   - the table entry, the affine predictor eta = shift + mult * p, its link and everything of the
//     density that does not depend on the row (1 / sigma^2, log sigma, exp(eta), the Bernoulli
//     softplus) are evaluated once per (group, particle), when the group changes: a row costs a
//     handful of FMAs;
//   - the row's value, mask, order and group are loaded kGsBatch rows ahead of their use;
//   - the sum of d log p / d eta over the group's rows stays in the lane (a float over one batch,
//     folded into a double) and is stored to dtable[k, g] when the group ends. Only the first and
//     the last group of a chunk can continue in a neighbour: those parts go to a slab
//     [role][end][chunk][K] and k_gather_tables adds them in chunk order; it also writes the zeros
//     of the groups without rows;
//   - the sums over all rows (the value, PARTICLE roles, shifts, mults) are kept per lane the same
//     way, written per (chunk, particle) and added in chunk order by k_gather_sums. d / d shift is
//     the sum of the group sums and d / d mult that of p times them: no work per row.
// Nothing is accumulated with atomics and every sum has a fixed order: two launches give the same
// bits. The Poisson rows' -lgamma(y + 1) does not depend on the particle: the first particle tile
// evaluates it once per row (rows dealt over the lanes) and adds the lanes' parts per chunk with a
// __shfl_xor butterfly, the one cross-lane sum of the kernel (its order is fixed too).
// Precondition: sorted_group is non-decreasing, its out-of-range entries included (k_gather_tables
// finds a group's rows by binary search). An unsorted array is never an address out of bounds,
// but its sums are undefined.
#include "gather_common.hpp"

namespace mi {

// Grid: x over blocks of kGsWaves * (64 >> ktl) chunks, y over tiles of 1 << ktl particles.
template <int FAMILY>
__global__ __launch_bounds__(kGsThreads) void k_gather_site(const mi_gather_site L, const GsWork W,
                                                            int ktl, double gscale,
                                                            uint32_t* __restrict__ flags) {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int KT = 1 << ktl;
  const int sub = lane >> ktl, kk = lane & (KT - 1);
  const int64_t K = L.K, N = L.N, G = L.G;
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
  const bool anydata = rowdata[0] || rowdata[1];
  const bool head_shared = cin && j0 > 0 && sg[j0 - 1] == sg[j0];
  const bool tail_shared = cin && j1 < N && sg[j1] == sg[j1 - 1];

  GsTerms<FAMILY> T;
  T.a0 = fixed[0];
  T.a1 = fixed[1];
  T.eta0 = 0.0f;
  float chain[2] = {1.0f, 1.0f};   // d role / d eta of a GATHER role
  GsAcc seg[2], lpacc, rolacc[2];
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
    float vv[kGsBatch], d0v[kGsBatch], d1v[kGsBatch];
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
      vv[u] = gs_value(L, o);
      const bool m = L.mask == nullptr || L.mask[o * L.mask_stride_i] != 0;
      d0v[u] = rowdata[0] ? L.role[0].data[o * L.role[0].stride_g] : 0.0f;
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
      }
      if (changed || anydata) {
        bool bad_eta = false;
        float a[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          a[r] = rowdata[r] ? (r == 0 ? d0v[u] : d1v[u]) : fixed[r];
          chain[r] = 1.0f;
          if (gathered[r]) {
            if (changed)
              praw[r] = gvalid ? L.role[r].data[k * L.role[r].stride_k + (int64_t)g * L.role[r].stride_g]
                               : 0.0f;
            const float eta = fmaf(mult[r], praw[r], shift[r]);
            bad_eta = bad_eta || gs_non_finite(eta);
            a[r] = eta;
            if (L.role[r].link == MI_GATHER_LINK_EXP) {
              a[r] = fast_exp(eta);
              if (FAMILY != MI_POISSON) chain[r] = a[r];
            }
            if (r == 0) T.eta0 = eta;
          }
        }
        T.a0 = a[0];
        T.a1 = a[1];
        T.derive(bad_eta);
      }
      if (ob[u]) {
        float lp, d0, d1;
        T.row(vv[u], lp, d0, d1);
        lpacc.add(lp);
        fl |= (T.bad ? MI_FLAG_PARAM : 0u) | (T.unsupported(vv[u]) ? MI_FLAG_SUPPORT : 0u);
        if (gathered[0]) seg[0].add(d0 * chain[0]);
        else rolacc[0].add(d0);
        if (FAMILY == MI_NORMAL) {
          if (gathered[1]) seg[1].add(d1 * chain[1]);
          else rolacc[1].add(d1);
        }
      }
    }
    seg[0].fold();
    seg[1].fold();
    lpacc.fold();
    rolacc[0].fold();
    rolacc[1].fold();
  }
  if (started) flush(true);

  if (cin && kin) {
    float* const base = W.sums + chunk * K + k;
    const int64_t plane = W.nchunk * K;
    base[0] = (float)lpacc.take();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (W.slot_role[r] >= 0) base[W.slot_role[r] * plane] = (float)rolacc[r].take();
      if (W.slot_shift[r] >= 0) base[W.slot_shift[r] * plane] = (float)dshift[r];
      if (W.slot_mult[r] >= 0) base[W.slot_mult[r] * plane] = (float)dmult[r];
    }
  }
  publish_flags(flags, fl);
}

// out[slot][k] = scale * sum_chunks sums[slot][chunk][k], chunks ascending (fp64); slot 0 is the
// value (plus the Poisson rows' constants) times site_scale, the others gradients times gscale.
// A block takes 32 particles of one slot; its kGsParts thread rows take every kGsParts-th chunk and
// meet in LDS, added in their order.
constexpr int kGsParts = 32;
__global__ __launch_bounds__(32 * kGsParts) void k_gather_sums(const GsWork W, int64_t K, double site_scale,
                                                     double gscale, int poisson) {
  __shared__ double red[kGsParts][32];
  const int kq = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int slot = blockIdx.y;
  const int64_t k = (int64_t)blockIdx.x * 32 + kq;
  double v = 0.0;
  if (k < K && W.out[slot] != nullptr) {
    const float* src = W.sums + (int64_t)slot * W.nchunk * K + k;
    for (int64_t c = part; c < W.nchunk; c += kGsParts) v += (double)src[c * K];
    if (slot == 0 && poisson)
      for (int64_t c = part; c < W.nchunk; c += kGsParts) v += W.rowc[c];
  }
  red[part][kq] = v;
  __syncthreads();
  if (part == 0 && k < K && W.out[slot] != nullptr) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < kGsParts; ++p) s += red[p][kq];
    W.out[slot][k] = (float)((slot == 0 ? site_scale : gscale) * s);
  }
}

// dtable[k, g] of the groups the site kernel did not store itself: 0 for a group without rows, the
// slab's parts in chunk order for a group whose rows span chunks. Grid: x over groups, y over
// particles, z over the GATHER roles with a dtable.
__global__ __launch_bounds__(256) void k_gather_tables(const mi_gather_site L, const GsWork W,
                                                       double gscale, int role0, int role1) {
  const int r = blockIdx.z == 0 ? role0 : role1;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (g >= L.G) return;
  const int32_t* __restrict__ const sg = L.sorted_group;
  int64_t lo, hi;
  gs_group_rows(sg, L.N, g, lo, hi);
  float* const dst = W.dtable[r] + k * L.G + g;
  if (lo == hi) {
    *dst = 0.0f;
    return;
  }
  const int64_t c0 = lo / kGsRows, c1 = (hi - 1) / kGsRows;
  if (c0 == c1) return;   // stored by the chunk that holds all its rows
  const float mult = gs_mult(L.role[r], k);
  // the chunk where the group starts left its tail, every later one its head
  double S = (double)W.slab[(((int64_t)r * 2 + 1) * W.nchunk + c0) * L.K + k];
  for (int64_t c = c0 + 1; c <= c1; ++c) S += (double)W.slab[(((int64_t)r * 2) * W.nchunk + c) * L.K + k];
  *dst = (float)(gscale * (double)mult * S);
}

// (gather_common.hpp)
int gs_finish(const mi_gather_site* site, const GsWork& W, double gscale, const int table_roles[2],
              int ntables, hipStream_t s) {
  hipError_t e;
  hipLaunchKernelGGL(k_gather_sums, dim3((unsigned)ceil_div(site->K, 32), (unsigned)W.nsum),
                     dim3(32 * kGsParts), 0, s, W, site->K, site->site_scale, gscale,
                     site->family == MI_POISSON ? 1 : 0);
  if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  if (ntables > 0) {
    hipLaunchKernelGGL(k_gather_tables,
                       dim3((unsigned)ceil_div(site->G, 256), (unsigned)site->K, (unsigned)ntables),
                       dim3(256), 0, s, *site, W, gscale, table_roles[0], table_roles[ntables - 1]);
    if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  }
  return 0;
}

}  // namespace mi

extern "C" {

int mi_gather_site_struct_size(size_t* bytes) {
  if (bytes == nullptr) return MI_EINVAL;
  *bytes = sizeof(mi_gather_site);
  return 0;
}

int mi_gather_site_workspace_bytes(const mi_gather_site* site, size_t* bytes) {
  if (!mi::gs_valid(site) || bytes == nullptr) return MI_EINVAL;
  *bytes = mi::gs_layout(site).bytes();
  return 0;
}

int mi_gather_site_forward(const mi_gather_site* site, void* workspace, size_t workspace_bytes,
                           float* total, const mi_gather_grads* grads, uint32_t* flags,
                           void* stream) {
  if (!mi::gs_valid(site) || total == nullptr || flags == nullptr) return MI_EINVAL;
  const mi::GsLayout y = mi::gs_layout(site);
  const mi::GsGrid g = mi::gs_grid(site, y);
  if (!mi::gs_supported(site, g)) return MI_EUNSUPPORTED;
  if (workspace == nullptr || workspace_bytes < y.bytes()) return MI_EWORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (!(site->options & MI_GROUP_FLAGS_ZEROED)) {
    if ((e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s)) != hipSuccess) return to_code(e);
  }
  mi::GsWork W{};
  int table_roles[2];
  const int ntables = mi::gs_bind(site, y, workspace, total, grads, W, table_roles);
  const double gscale = (double)site->grad_scale * site->site_scale;
  const dim3 grid((unsigned)g.gx, (unsigned)g.gy);
  const int ktl = g.ktl;
  if (site->family == MI_NORMAL)
    hipLaunchKernelGGL((mi::k_gather_site<MI_NORMAL>), grid, dim3(mi::kGsThreads), 0, s, *site, W, ktl,
                       gscale, flags);
  else if (site->family == MI_BERNOULLI_LOGITS)
    hipLaunchKernelGGL((mi::k_gather_site<MI_BERNOULLI_LOGITS>), grid, dim3(mi::kGsThreads), 0, s, *site,
                       W, ktl, gscale, flags);
  else
    hipLaunchKernelGGL((mi::k_gather_site<MI_POISSON>), grid, dim3(mi::kGsThreads), 0, s, *site, W, ktl,
                       gscale, flags);
  if ((e = hipGetLastError()) != hipSuccess) return to_code(e);
  return mi::gs_finish(site, W, gscale, table_roles, ntables, s);
}

}  // extern "C"
