// Site log-probability accumulation over the particle x element space of a model trace.
//
// Replaces, for the Normal / Bernoulli / Beta / Categorical families, the per-site
// `distribution.log_prob(value)` of the reference tracer (mininf/core.py:241, masked branch
// core.py:231-239), the per-site sums and minibatch scaling of LogProbTracer.total/contribution
// (core.py:247-273) and the autograd backward of those torch ops. Formulas restate
// torch/distributions (file:line cited at each family below).
//
// Three launch shapes, chosen on the host from the operand strides (mi_group_forward):
//   ROW   -- a dense operand is contiguous along elements (x[k, i], stride_i == 1): lanes run along
//            i, each wave owns a 64*ELEMS element segment and walks particle rows; coalesced
//            256-B loads/stores per wave instruction; per-row wave-shuffle reduction.
//   COL   -- a dense operand is contiguous along particles (x[i, k] as produced by a vmapped
//            `X @ theta`, stride_k == 1) or there is no dense operand: lanes run along k and loop
//            over elements; per-lane accumulation, no cross-lane reduction per element.
//   BCAST -- one site whose parameters are per-particle scalars and whose value is shared data
//            x[i] (the biased-coin / C2 shape): the value chunk is staged once in LDS and read as
//            a broadcast float4 while each lane owns P particles; the per-particle constant part of
//            log p is hoisted out of the element loop, leaving one FMA per (particle, element).
// All three write per-(segment, particle) partial sums (fp32) that k_finalize (reduce.hip) reduces
// in fp64 in a fixed order, so results are deterministic run to run.
// The BCAST kernels and their launch policy are in bcast_site.hip (this unit plans with
// bcast_site.hpp), k_finalize and the other shared reductions in reduce.hip.
#include "common.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bcast_site.hpp"
#include "internal.hpp"
#include "jit.hpp"
namespace mi {

// Uniform (scalar-branch) selection from compile-time-indexed register arrays; `idx` is always
// wave-uniform (it comes from the kernel argument block), so no VALU select chains are emitted.
template <int N>
MI_DEV float pick(const float (&v)[N], int idx) {
  float out = 0.0f;
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (idx == j) out = v[j];
  return out;
}

template <int N>
MI_DEV void add_at(float (&v)[N], int idx, float x) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (idx == j) v[j] += x;
}

// One (particle k, element i) of a site group: loads every operand once, evaluates every site,
// accumulates per-site log p and per-slot particle gradients, writes dense operand gradients.
MI_DEV void group_element(const mi_group& G, int64_t k, int64_t i, float (&lp)[MI_MAX_SITES],
                          float (&slot)[MI_MAX_SLOTS], uint32_t (&fl)[MI_MAX_SITES]) {
  float ov[MI_MAX_OPERANDS];
  float og[MI_MAX_OPERANDS];
#pragma unroll
  for (int o = 0; o < MI_MAX_OPERANDS; ++o) {
    og[o] = 0.0f;
    ov[o] = 0.0f;
    if (o < G.num_operands) {
      const mi_operand& op = G.operands[o];
      ov[o] = op.data[k * op.stride_k + i * op.stride_i];
    }
  }
#pragma unroll
  for (int s = 0; s < MI_MAX_SITES; ++s) {
    if (s < G.num_sites) {
      const mi_site& st = G.sites[s];
      float r[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) r[q] = st.operand[q] < 0 ? st.constant[q] : pick(ov, st.operand[q]);
      bool observed = true;
      if (st.mask != nullptr) observed = st.mask[k * st.mask_stride_k + i * st.mask_stride_i] != 0;
      Elem e;
      eval_family(st.family, r[0], r[1], r[2], st.extra, e);
      lp[s] += observed ? e.lp : 0.0f;
      fl[s] |= (e.param_bad ? MI_FLAG_PARAM : 0u) | ((observed && e.support_bad) ? MI_FLAG_SUPPORT : 0u);
      if (G.compute_grads) {
        const float w = observed ? (float)st.scale : 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int o = st.operand[q];
          if (o >= 0) {
            const int mode = G.operands[o].grad_mode;
            if (mode == MI_GRAD_DENSE) add_at(og, o, w * e.d[q]);
            else if (mode == MI_GRAD_PARTICLE) add_at(slot, G.operands[o].slot, w * e.d[q]);
          }
        }
      }
    }
  }
  if (G.compute_grads) {
#pragma unroll
    for (int o = 0; o < MI_MAX_OPERANDS; ++o) {
      if (o < G.num_operands) {
        const mi_operand& op = G.operands[o];
        if (op.grad_mode == MI_GRAD_DENSE)
          op.grad[k * op.grad_stride_k + i * op.grad_stride_i] = G.grad_scale * og[o];
      }
    }
  }
}

// Partial sums layout: part[(v * nseg + seg) * K + k] for value v in
// [0, num_sites) (per-site log p) followed by [num_sites, num_sites + num_slots) (slot grads).

// -------------------------------------------------------------------------------------------------
// ROW: lanes along elements.
// -------------------------------------------------------------------------------------------------
template <int ELEMS>
__global__ __launch_bounds__(256) void k_group_row(const mi_group G, float* __restrict__ part,
                                                   int64_t nseg, int64_t rows_per_block,
                                                   uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  uint32_t fl[MI_MAX_SITES] = {0u, 0u, 0u, 0u};
  if (seg < nseg) {
    const int64_t base = seg * (64 * ELEMS);
    const int64_t k_begin = (int64_t)blockIdx.y * rows_per_block;
    const int64_t k_end = min(G.K, k_begin + rows_per_block);
    const int nv = G.num_sites + G.num_slots;
    for (int64_t kb = k_begin; kb < k_end; kb += 64) {
      float keep[MI_MAX_SITES + MI_MAX_SLOTS];
#pragma unroll
      for (int v = 0; v < MI_MAX_SITES + MI_MAX_SLOTS; ++v) keep[v] = 0.0f;
      const int rows = (int)min((int64_t)64, k_end - kb);
      for (int r = 0; r < rows; ++r) {
        const int64_t k = kb + r;
        float lp[MI_MAX_SITES] = {0.f, 0.f, 0.f, 0.f};
        float slot[MI_MAX_SLOTS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < ELEMS; ++e) {
          const int64_t i = base + e * 64 + lane;
          if (i < G.N) group_element(G, k, i, lp, slot, fl);
        }
#pragma unroll
        for (int s = 0; s < MI_MAX_SITES; ++s) {
          if (s < G.num_sites) {
            const float t = wave_sum(lp[s]);
            keep[s] = (lane == r) ? t : keep[s];
          }
        }
#pragma unroll
        for (int j = 0; j < MI_MAX_SLOTS; ++j) {
          if (j < G.num_slots) {
            const float t = wave_sum(slot[j]);
            keep[MI_MAX_SITES + j] = (lane == r) ? t : keep[MI_MAX_SITES + j];
          }
        }
      }
      if (lane < rows) {
#pragma unroll
        for (int s = 0; s < MI_MAX_SITES; ++s)
          if (s < G.num_sites) part[((int64_t)s * nseg + seg) * G.K + kb + lane] = keep[s];
#pragma unroll
        for (int j = 0; j < MI_MAX_SLOTS; ++j)
          if (j < G.num_slots)
            part[((int64_t)(G.num_sites + j) * nseg + seg) * G.K + kb + lane] = keep[MI_MAX_SITES + j];
      }
      (void)nv;
    }
  }
#pragma unroll
  for (int s = 0; s < MI_MAX_SITES; ++s)
    if (s < G.num_sites) publish_flags(flags + s, fl[s]);
}

// -------------------------------------------------------------------------------------------------
// COL: lanes along particles. `kw` lanes (power of two <= 64) cover consecutive particles, the
// 64 / kw lane groups of a wave take interleaved elements.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_group_col(const mi_group G, float* __restrict__ part,
                                                   int64_t nseg, int64_t seg_len, int kw,
                                                   uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int kq = lane & (kw - 1);
  const int isub = lane / kw;
  const int istep = 64 / kw;
  const int64_t k = (int64_t)blockIdx.y * kw + kq;
  uint32_t fl[MI_MAX_SITES] = {0u, 0u, 0u, 0u};
  float lp[MI_MAX_SITES] = {0.f, 0.f, 0.f, 0.f};
  float slot[MI_MAX_SLOTS] = {0.f, 0.f, 0.f, 0.f};
  if (seg < nseg && k < G.K) {
    const int64_t i_begin = seg * seg_len;
    const int64_t i_end = min(G.N, i_begin + seg_len);
#pragma unroll 4
    for (int64_t i = i_begin + isub; i < i_end; i += istep) group_element(G, k, i, lp, slot, fl);
  }
  if (kw < 64) {
#pragma unroll
    for (int s = 0; s < MI_MAX_SITES; ++s)
      if (s < G.num_sites) lp[s] = wave_sum_strided(lp[s], kw);
#pragma unroll
    for (int j = 0; j < MI_MAX_SLOTS; ++j)
      if (j < G.num_slots) slot[j] = wave_sum_strided(slot[j], kw);
  }
  if (seg < nseg && k < G.K && isub == 0) {
#pragma unroll
    for (int s = 0; s < MI_MAX_SITES; ++s)
      if (s < G.num_sites) part[((int64_t)s * nseg + seg) * G.K + k] = lp[s];
#pragma unroll
    for (int j = 0; j < MI_MAX_SLOTS; ++j)
      if (j < G.num_slots) part[((int64_t)(G.num_sites + j) * nseg + seg) * G.K + k] = slot[j];
  }
#pragma unroll
  for (int s = 0; s < MI_MAX_SITES; ++s)
    if (s < G.num_sites) publish_flags(flags + s, fl[s]);
}

}  // namespace mi

// =================================================================================================
// Host side: launch-shape selection and the C ABI.
// =================================================================================================
namespace {

using mi::bcast_eligible;
using mi::bcast_smem;
using mi::kSmemP;
using mi::smem_rank1;

enum Shape { kRow = 0, kCol = 1, kBcast = 2 };

constexpr int kRowElems = 8;
constexpr int kColUnroll = 4;
constexpr int64_t kTargetBlocks = 2048;

bool validate_group(const mi_group* g) {
  if (g == nullptr || g->K < 1 || g->N < 1) return false;
  if (g->num_sites < 1 || g->num_sites > MI_MAX_SITES) return false;
  if (g->num_operands < 0 || g->num_operands > MI_MAX_OPERANDS) return false;
  if (g->num_slots < 0 || g->num_slots > MI_MAX_SLOTS) return false;
  for (int s = 0; s < g->num_sites; ++s) {
    const mi_site& st = g->sites[s];
    if (st.family < MI_NORMAL || st.family > MI_NEGATIVE_BINOMIAL) return false;
    if (st.operand[2] < 0) return false;  // the value is always an operand
    for (int q = 0; q < 3; ++q)
      if (st.operand[q] >= g->num_operands) return false;
  }
  const int draw = g->draw.operand - 1;
  if (draw >= g->num_operands || draw < -1) return false;
  if (draw >= 0 && (g->draw.loc == nullptr || g->draw.scale == nullptr ||
                    g->draw.element_offset < 0 || (g->draw.element_offset & 3) != 0 ||
                    (g->compute_grads && !(g->options & MI_GROUP_DRAW_PARTIALS) &&
                     (g->draw.dloc == nullptr || g->draw.dscale == nullptr))))
    return false;
  if (g->side.out != nullptr &&
      (g->side.x == nullptr || g->side.c1 == nullptr || g->side.c0 == nullptr || g->side.K < 1 ||
       g->side.N < 1))
    return false;
  if (g->prior.present != 0 &&
      ((g->prior.family != MI_BETA && g->prior.family != MI_NORMAL && g->prior.family != MI_GAMMA) ||
       g->prior.flags == nullptr || g->sites[0].operand[0] < 0))
    return false;
  const int pdraw = g->pdraw.operand - 1;
  if (pdraw >= g->num_operands || pdraw < -1 || (pdraw >= 0 && pdraw == draw)) return false;
  if (pdraw >= 0 && (g->pdraw.loc == nullptr || g->pdraw.scale == nullptr ||
                     g->pdraw.element_offset < 0 || (g->pdraw.element_offset & 3) != 0 ||
                     g->operands[pdraw].stride_i != 0 || g->operands[pdraw].stride_k == 0))
    return false;
  for (int o = 0; o < g->num_operands; ++o) {
    const mi_operand& op = g->operands[o];
    if (o == draw) continue;  // computed in the kernel
    if (op.data == nullptr) return false;
    if (op.grad_mode == MI_GRAD_DENSE && op.grad == nullptr) return false;
    if (op.grad_mode == MI_GRAD_PARTICLE && (op.slot < 0 || op.slot >= g->num_slots)) return false;
  }
  return true;
}

// A fused guide draw (mi_draw) needs the row layout with whole element quads per lane and plain
// row-major [K, N] companions (see include/mininf_amd.h).
// Largest particle block of a program that makes a per-particle draw (mi_group.pdraw): the
// values live in an LDS table of the program (jit.cpp kPdrawTable).
constexpr int64_t kPdrawMax = 1024;

bool draw_supported(const mi_group* g) {
  const int draw = g->draw.operand - 1;
  if (draw < 0) return true;
  if (g->N % 4 != 0 || g->N < 64 * 8) return false;
  for (int o = 0; o < g->num_operands; ++o) {
    const mi_operand& op = g->operands[o];
    if (o == draw) continue;
    if (op.stride_k != 0 && op.stride_i != 0 && op.stride_i != 1) return false;
    if (op.stride_k == 0 && op.stride_i != 0 && op.stride_i != 1) return false;
  }
  for (int s = 0; s < g->num_sites; ++s) {
    const mi_site& st = g->sites[s];
    if (st.mask != nullptr && st.mask_stride_k != 0) return false;
  }
  return true;
}

bool is_dense(const mi_operand& op) { return op.stride_k != 0 && op.stride_i != 0; }

struct Plan {
  Shape shape;
  bool draw = false;       // a fused guide draw (mi_draw)
  int elems;               // ROW: elements per lane per row
  int64_t nseg;
  int64_t rows_per_block;  // ROW
  int64_t seg_len;         // COL
  int kw;                  // COL
  int chunk = 0;           // BCAST (k_site_bcast_smem): elements per chunk
  dim3 grid;
};

Plan make_plan(const mi_group* g) {
  Plan p{};
  if (g->draw.operand == 0 && bcast_eligible(g)) {
    p.shape = kBcast;
    const bool smem = bcast_smem(g);
    if (smem) p.chunk = mi::smem_chunk(g->N, ceil_div(g->K, mi::kBcastThreads * kSmemP));
    const int64_t chunks = ceil_div(g->N, smem ? p.chunk : mi::kBcastChunk);
    p.nseg = smem ? chunks + 1 : chunks;   // k_site_bcast_smem: + the particle-constant segment
    const int64_t side = smem ? mi::beta_side_blocks(g->side) : 0;
    p.grid = dim3((unsigned)(chunks + side),
                  (unsigned)ceil_div(g->K, mi::kBcastThreads * (smem ? kSmemP : mi::kBcastP)));
    return p;
  }
  int dense = -1;
  for (int o = 0; o < g->num_operands; ++o)
    if (is_dense(g->operands[o])) { dense = o; break; }
  const bool row = dense >= 0 && g->operands[dense].stride_i == 1 && g->operands[dense].stride_k != 1;
  const bool row_fallback = dense >= 0 && g->operands[dense].stride_k != 1 && g->operands[dense].stride_i != 1 &&
                            llabs(g->operands[dense].stride_i) < llabs(g->operands[dense].stride_k);
  // Short element spaces (e.g. a prior over a handful of coefficients) have too few row
  // segments to fill the chip and would loop over all particles serially: lanes go along
  // particles instead.
  const bool short_rows = g->N < 256 && g->draw.operand == 0;
  if ((row || row_fallback) && !short_rows) {
    p.shape = kRow;
    p.draw = g->draw.operand != 0;
    // fused draws: one Philox quad per lane and row keeps the register footprint at 4 waves/SIMD
    p.elems = g->draw.operand != 0 ? 4 : kRowElems;
    p.nseg = ceil_div(g->N, 64 * p.elems);
    const int64_t gx = ceil_div(p.nseg, 4);
    // about two rounds of 4-wave blocks (fused draws: fewer, longer particle blocks write fewer
    // d loc / d scale partial rows for the same balance; r04/r05 sweeps kept this target)
    int64_t gy = std::max<int64_t>(1, std::min<int64_t>(ceil_div(g->K, 64),
                                                        ceil_div(kTargetBlocks, gx)));
    p.rows_per_block = ceil_div(g->K, gy);
    gy = ceil_div(g->K, p.rows_per_block);
    p.grid = dim3((unsigned)gx, (unsigned)gy);
    return p;
  }
  p.shape = kCol;
  int kw = 1;
  while (kw < 64 && kw < g->K) kw <<= 1;
  p.kw = kw;
  const int64_t gy = ceil_div(g->K, kw);
  const int istep = 64 / kw;
  const int64_t waves_per_tile = std::max<int64_t>(1, (kTargetBlocks * 4) / gy);
  int64_t seg_len = ceil_div(g->N, waves_per_tile);
  seg_len = std::max<int64_t>(seg_len, (int64_t)istep * 16);
  seg_len = ceil_div(seg_len, istep) * istep;
  p.seg_len = seg_len;
  p.nseg = ceil_div(g->N, seg_len);
  p.grid = dim3((unsigned)ceil_div(p.nseg, 4), (unsigned)gy);
  return p;
}

PlanInfo plan_info(const Plan& p, bool combined) {
  PlanInfo info{};
  info.combined = combined;
  info.row = p.shape == kRow;
  info.elems = p.shape == kRow ? p.elems : kColUnroll;
  // fused draws: the block's four waves combine their particle sums (a quarter of the partial rows:
  // C5's 3907 segments become 977 rows, within the ELBO forward's fused reduction)
  info.block_rows = info.row && p.draw;
  info.packed = info.row && p.draw;
  info.kw = p.kw;
  info.grid_x = p.grid.x;
  info.grid_y = p.grid.y;
  return info;
}

// Particle-summed site values (MI_GROUP_KSUM): a k_site_bcast_smem launch whose reduction the
// ELBO forward can take (a deferrable segment list) over at most MI_KSUM_MAX_K particles (the
// forward then reduces such a job in a few hundred blocks at most).
bool use_ksum(const mi_group* g, const Plan& p) {
  return (g->options & MI_GROUP_KSUM) && p.shape == kBcast && bcast_smem(g) &&
         p.nseg <= MI_REDUCE_MAX_SEG && g->K >= 4 && g->K <= MI_KSUM_MAX_K;
}

// The doubles such a launch writes: one per (chunk, particle block), then one per workgroup that
// evaluates the particle-constant segment (k_site_bcast_smem).
int64_t ksum_doubles(const Plan& p) {
  const int64_t chunks = p.nseg - 1;
  return (chunks + (chunks >= kSmemP ? kSmemP : 1)) * (int64_t)p.grid.y;
}

// The [nseg, K] fp32 blocks of the values (without the site value's when it is particle-summed).
size_t slab_bytes(const mi_group* g, const Plan& p) {
  const int nv = g->num_sites + g->num_slots - (use_ksum(g, p) ? 1 : 0);
  return (size_t)nv * (size_t)p.nseg * (size_t)g->K * sizeof(float);
}

// Particle-summed values: the doubles follow the (256-byte aligned) blocks.
size_t ksum_offset(const mi_group* g, const Plan& p) { return (slab_bytes(g, p) + 255) / 256 * 256; }

size_t partial_bytes(const mi_group* g, const Plan& p) {
  if (!use_ksum(g, p)) return slab_bytes(g, p);
  return ksum_offset(g, p) + (size_t)ksum_doubles(p) * sizeof(double);
}

// BCAST groups also hold the per-particle constants after the (256-byte aligned) partials.
size_t prep_offset(const mi_group* g, const Plan& p) {
  return (partial_bytes(g, p) + 255) / 256 * 256;
}

// Per-K-block partial dloc / dscale of a fused draw (when the grid splits the particles, or when
// the caller reduces them itself: MI_GROUP_DRAW_PARTIALS).
size_t draw_partial_floats(const mi_group* g, const Plan& p) {
  if (g->draw.operand == 0 || !g->compute_grads) return 0;
  if (p.grid.y <= 1 && !(g->options & MI_GROUP_DRAW_PARTIALS)) return 0;
  return 2 * (size_t)p.grid.y * (size_t)g->N;
}

size_t finalize_offset(const mi_group* g, const Plan& p) {
  const size_t middle = p.shape != kBcast ? draw_partial_floats(g, p) * sizeof(float)
                                          : (size_t)mi::kPrep * (size_t)g->K * sizeof(float);
  return (prep_offset(g, p) + middle + 255) / 256 * 256;
}

size_t workspace_bytes(const mi_group* g, const Plan& p) {
  return finalize_offset(g, p) +
         mi_finalize_scratch_bytes(p.nseg, g->K, g->num_sites + g->num_slots);
}

// What a group may ask for beyond its sites, each in the shape that provides it: a fused draw (a
// ROW site program), a side job (k_site_bcast_smem), a folded prior, a per-particle draw.
bool extras_supported(const mi_group* group, const Plan& p, bool combined) {
  if (group->draw.operand != 0 && (p.shape != kRow || !draw_supported(group))) return false;
  if (group->side.out != nullptr && !(p.shape == kBcast && bcast_smem(group))) return false;
  int ok = 1;
  if (group->prior.present != 0) {
    mi_group_prior_supported(group, &ok);
    if (!ok || (p.shape == kRow && !combined)) return false;
  }
  if (group->pdraw.operand != 0) mi_group_pdraw_supported(group, &ok);
  return ok != 0;
}

// ROW / COL: the site program specialised for the group (jit.cpp; `specialised`) or, where there
// is no specialiser, the generic kernel. `draw_partials` (or NULL): where a fused draw's per-K-block
// d loc / d scale partials go. Returns 0, an MI_E* code or a hipError_t.
int launch_row_col(const mi_group& G, const Plan& p, const PlanInfo& info, float* draw_partials,
                   float* part, uint32_t* flags, hipStream_t s, bool* specialised) {
  mi_group GK = G;
  if (draw_partials != nullptr) {
    GK.draw.dloc = draw_partials;
    GK.draw.dscale = draw_partials + (size_t)p.grid.y * G.N;
  }
  const int rc = mi_jit_launch(GK, info, part, p.nseg,
                               p.shape == kRow ? p.rows_per_block : p.seg_len, flags, s);
  if (rc < 0) return -rc;
  *specialised = rc == 0;
  if (rc == 0) return 0;
  if (G.draw.operand != 0) return MI_EUNSUPPORTED;  // fused draws need the specialised kernel
  if (p.shape == kCol)
    hipLaunchKernelGGL(mi::k_group_col, p.grid, dim3(256), 0, s, G, part, p.nseg, p.seg_len, p.kw,
                       flags);
  else if (p.elems == 4)
    hipLaunchKernelGGL((mi::k_group_row<4>), p.grid, dim3(256), 0, s, G, part, p.nseg,
                       p.rows_per_block, flags);
  else if (p.elems == 16)
    hipLaunchKernelGGL((mi::k_group_row<16>), p.grid, dim3(256), 0, s, G, part, p.nseg,
                       p.rows_per_block, flags);
  else
    hipLaunchKernelGGL((mi::k_group_row<8>), p.grid, dim3(256), 0, s, G, part, p.nseg,
                       p.rows_per_block, flags);
  return 0;
}

}  // namespace

extern "C" {

int mi_abi_version(char* target, size_t target_bytes) {
  const char name[] = "gfx950";
  if (target != nullptr && target_bytes > 0) {
    size_t n = 0;
    for (; n + 1 < target_bytes && name[n] != '\0'; ++n) target[n] = name[n];
    target[n] = '\0';
  }
  return MI_ABI_VERSION;
}

int mi_wall_clock_khz(int* khz) {
  if (khz == nullptr) return MI_EINVAL;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(khz, hipDeviceAttributeWallClockRate, dev);
  return to_code(e);
}

int mi_struct_sizes(size_t* operand, size_t* site, size_t* group) {
  if (operand == nullptr || site == nullptr || group == nullptr) return MI_EINVAL;
  *operand = sizeof(mi_operand);
  *site = sizeof(mi_site);
  *group = sizeof(mi_group);
  return 0;
}

int mi_group_side_supported(const mi_group* group, int* supported) {
  if (!validate_group(group) || supported == nullptr) return MI_EINVAL;
  const Plan p = make_plan(group);
  *supported = (p.shape == kBcast && bcast_smem(group)) ? 1 : 0;
  return 0;
}

int mi_group_prior_supported(const mi_group* group, int* supported) {
  if (!validate_group(group) || supported == nullptr) return MI_EINVAL;
  const Plan p = make_plan(group);
  // the BCAST kernel's one site, or a fused-draw site program's site 0 (evaluated at its
  // block-row flush); either way on site 0's per-particle parameter, an operand (stride_i == 0)
  const int o = group->sites[0].operand[0];
  const bool host = (p.shape == kBcast && bcast_smem(group) && group->num_sites == 1) ||
                    (p.shape == kRow && p.draw && draw_supported(group) && mi_jit_enabled());
  *supported = (host && o >= 0 && group->operands[o].stride_i == 0 &&
                group->operands[o].stride_k != 0 &&
                group->prior.scale == group->sites[0].scale) ? 1 : 0;
  return 0;
}

int mi_group_pdraw_supported(const mi_group* group, int* supported) {
  if (!validate_group(group) || supported == nullptr) return MI_EINVAL;
  const Plan p = make_plan(group);
  // a fused-draw site program (row shape, block-row partials) whose particle block fits the
  // program's LDS table of per-particle values
  *supported = (p.shape == kRow && p.draw && draw_supported(group) && mi_jit_enabled() &&
                p.rows_per_block <= kPdrawMax) ? 1 : 0;
  return 0;
}

int mi_group_workspace_bytes(const mi_group* group, size_t* bytes) {
  if (!validate_group(group) || bytes == nullptr) return MI_EINVAL;
  const Plan p = make_plan(group);
  *bytes = workspace_bytes(group, p);
  return 0;
}

int mi_group_forward(const mi_group* group, void* workspace, size_t workspace_bytes, float* total,
                     double* site_lp, float* slot_grad, uint32_t* flags, void* stream) {
  return mi_group_forward_deferred(group, workspace, workspace_bytes, total, site_lp, slot_grad,
                                   flags, nullptr, nullptr, stream, nullptr);
}

int mi_group_forward_deferred(const mi_group* group, void* workspace, size_t workspace_bytes,
                              float* total, double* site_lp, float* slot_grad, uint32_t* flags,
                              void* start_event, void* stop_event, void* stream,
                              mi_reduce* reduce) {
  if (reduce != nullptr) *reduce = mi_reduce{};
  if (!validate_group(group) || total == nullptr || flags == nullptr) return MI_EINVAL;
  if (group->num_slots > 0 && slot_grad == nullptr) return MI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (start_event != nullptr || stop_event != nullptr) {   // eager timing only (internal.hpp)
    bool capturing = false;
    const hipError_t ce = mi_stream_capturing(s, &capturing);
    if (ce != hipSuccess) return to_code(ce);
    if (capturing) return MI_EUNSUPPORTED;
  }
  const Plan p = make_plan(group);
  if (workspace_bytes < ::workspace_bytes(group, p) || workspace == nullptr) return MI_EWORKSPACE;
  // particle-summed values exist only for a caller that takes the reduction and wants no
  // per-particle site values (nothing is enqueued: the caller may launch again without the option)
  const bool ksummed = use_ksum(group, p);
  if (ksummed && (reduce == nullptr || site_lp != nullptr)) return MI_EUNSUPPORTED;
  char* ws = static_cast<char*>(workspace);
  double* ksum = ksummed ? reinterpret_cast<double*>(ws + ksum_offset(group, p)) : nullptr;
  float* part = static_cast<float*>(workspace);
  float* prep = reinterpret_cast<float*>(ws + prep_offset(group, p));
  hipError_t e = hipSuccess;
  if (!(group->options & MI_GROUP_FLAGS_ZEROED)) {
    e = hipMemsetAsync(flags, 0, sizeof(uint32_t) * group->num_sites, s);
    if (e == hipSuccess && group->prior.present != 0)
      e = hipMemsetAsync(group->prior.flags, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return to_code(e);
  }
  const mi_group G = *group;
  // Without a per-site output the specialised kernels reduce one weighted log-joint value per
  // particle instead of one per site.
  const bool combined = site_lp == nullptr;
  if (!extras_supported(group, p, combined)) return MI_EUNSUPPORTED;
  int reduced_lp = G.num_sites;
  bool prescaled = false;  // partials already carry the site scales
  int64_t prows = p.nseg;   // partial rows written (fused-draw programs: one per block)
  float* draw_partials = draw_partial_floats(group, p) != 0 ? prep : nullptr;
  const bool smem = p.shape == kBcast && bcast_smem(group);
  const bool plain = p.shape == kBcast && !smem;
  // (the prep-plus-site launch records it itself, behind its prep kernel)
  if (start_event != nullptr && !plain) {
    e = mi_record_event(start_event, s);
    if (e != hipSuccess) return to_code(e);
  }
  if (smem) {
    mi::bcast_launch_smem(G, part, p.nseg, p.grid, p.chunk, flags, ksum, s);
  } else if (plain) {
    const int rc = mi::bcast_launch(G, prep, part, p.nseg, p.grid, flags, start_event, s);
    if (rc != 0) return rc;
  } else {
    const PlanInfo info = plan_info(p, combined);
    bool specialised = false;
    const int rc = launch_row_col(G, p, info, draw_partials, part, flags, s, &specialised);
    if (rc != 0) return rc;
    if (specialised) {
      prescaled = combined;
      reduced_lp = combined ? 1 : G.num_sites;
      if (info.block_rows) prows = (int64_t)p.grid.x;
    }
  }
  e = hipGetLastError();
  if (e != hipSuccess) return to_code(e);
  if (stop_event != nullptr) {
    e = mi_record_event(stop_event, s);
    if (e != hipSuccess) return to_code(e);
  }
  if (draw_partials != nullptr && !(G.options & MI_GROUP_DRAW_PARTIALS)) {
    const int rc = mi_launch_draw_reduce(draw_partials, (int64_t)p.grid.y, G.N, G.draw.dloc,
                                         G.draw.dscale, s);
    if (rc != 0) return rc;
  }
  double scales[MI_MAX_SITES];
  for (int i = 0; i < reduced_lp; ++i) scales[i] = prescaled ? 1.0 : G.sites[i].scale;
  // values in the rank-one layout: the slot of a k_site_bcast_smem launch (after the site value)
  const int rank1_mask = (smem && smem_rank1(group, p.nseg)) ? (1 << reduced_lp) : 0;
  if (reduce != nullptr && prows <= MI_REDUCE_MAX_SEG) {   // the caller runs the finalize
    if (ksummed) {   // (the smem kernel's one site value)
      reduce->ksum = 1;   // (its doubles at ksum_offset: mi_reduce.ksum's convention)
      reduce->nksum = ksum_doubles(p);
    }
    reduce->part = part;
    reduce->nseg = prows;
    reduce->K = G.K;
    reduce->num_sites = reduced_lp;
    reduce->num_slots = G.num_slots;
    reduce->rank1 = rank1_mask;
    for (int i = 0; i < reduced_lp; ++i) reduce->scale[i] = scales[i];
    reduce->slot_scale = (double)G.grad_scale;
    reduce->total = total;
    reduce->site_lp = site_lp;
    reduce->slot_grad = slot_grad;
    return 0;
  }
  double* scratch = reinterpret_cast<double*>(ws + finalize_offset(group, p));
  return mi_launch_finalize(part, prows, G.K, reduced_lp, G.num_slots, scales,
                            (double)G.grad_scale, total, site_lp, slot_grad, scratch, s,
                            rank1_mask);
}

int mi_group_draw_partials(const mi_group* group, size_t* offset_bytes, int64_t* rows) {
  if (!validate_group(group) || offset_bytes == nullptr || rows == nullptr) return MI_EINVAL;
  if (!(group->options & MI_GROUP_DRAW_PARTIALS)) return MI_EINVAL;
  const Plan p = make_plan(group);
  if (draw_partial_floats(group, p) == 0) return MI_EINVAL;
  *offset_bytes = prep_offset(group, p);
  *rows = (int64_t)p.grid.y;
  return 0;
}

int mi_group_source(const mi_group* group, char* out, size_t out_bytes, size_t* needed) {
  if (!validate_group(group)) return MI_EINVAL;
  const Plan p = make_plan(group);
  std::string text;
  if (p.shape == kBcast) text = "// BCAST shape: precompiled k_site_bcast\n";
  else text = mi_jit_source(*group, plan_info(p, true));
  if (needed != nullptr) *needed = text.size() + 1;
  if (out != nullptr && out_bytes > 0) {
    const size_t n = std::min(out_bytes - 1, text.size());
    std::memcpy(out, text.data(), n);
    out[n] = '\0';
  }
  return 0;
}

int mi_group_compile_check(const mi_group* group, char* log, size_t log_bytes) {
  if (!validate_group(group)) return MI_EINVAL;
  const Plan p = make_plan(group);
  if (p.shape == kBcast) return 0;
  std::string text;
  const bool ok = mi_jit_compile_check(*group, plan_info(p, true), &text) &&
                  mi_jit_compile_check(*group, plan_info(p, false), &text);
  if (log != nullptr && log_bytes > 0) {
    const size_t n = std::min(log_bytes - 1, text.size());
    std::memcpy(log, text.data(), n);
    log[n] = '\0';
  }
  return ok ? 0 : MI_EUNSUPPORTED;
}

}  // extern "C"
