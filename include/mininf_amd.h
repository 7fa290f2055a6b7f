/*
 * mininf_amd.h -- C ABI of the MI355X (gfx950) ELBO hot path.
 *
 * The reference (tillahoffmann/mininf) is pure Python on PyTorch and has no FFI of its own; its
 * "operator API" for the ELBO path is three Python seams:
 *   1. the tracer plugin point  -- mininf/core.py:128-140 (TracerMixin.sample), dispatched from
 *      mininf/core.py:325-328 (sample);
 *   2. the Distribution protocol consumed at mininf/core.py:233-241 (log_prob) and
 *      mininf/nn.py:124-145, 217, 226 (rsample / entropy);
 *   3. the loss module mininf/nn.py:212-228 (EvidenceLowerBoundLoss.forward).
 * Every entry point below replaces the arithmetic behind one of those seams; the comment above each
 * one names the reference line(s) and the torch.distributions code it stands in for.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative MI_E* code for an invalid argument, or a positive hipError_t;
 *   - never throw across the ABI, never allocate device memory (workspaces are caller-provided and
 *     sized by the matching *_workspace_bytes query), never synchronise the host;
 *   - asynchronous on the given stream (`stream` is a hipStream_t; NULL = the null stream);
 *   - tensors are device pointers plus int64 element strides over a logical [K, N] space
 *     (K = Monte-Carlo particles, N = flattened elements of one site); a stride of 0 broadcasts;
 *   - floating-point data is IEEE fp32 (the reference's default dtype); accumulation is fp32
 *     within a wavefront and fp64 across wavefronts.
 */
#ifndef MININF_AMD_H
#define MININF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 18 also covers the particle-summed site values (MI_GROUP_KSUM, mi_reduce.ksum / nksum), which
 * grew mi_reduce and so mi_elbo: a caller built against the earlier 18 is told apart by
 * mi_elbo_struct_sizes (sizeof(mi_elbo)), which bindings must check beside this number. */
#define MI_ABI_VERSION 18

#define MI_MAX_SITES 4
#define MI_MAX_OPERANDS 6
#define MI_MAX_SLOTS 4

/* error codes (negative) */
#define MI_EINVAL (-1)      /* malformed descriptor or size */
#define MI_EWORKSPACE (-2)  /* workspace too small */
#define MI_EUNSUPPORTED (-3)

/* site families (torch.distributions formulas they restate are cited in sites.hip) */
enum mi_family {
  MI_NORMAL = 0,            /* roles: loc, scale, value          torch/distributions/normal.py:88-103 */
  MI_BERNOULLI_LOGITS = 1,  /* roles: logits, -, value            torch/distributions/bernoulli.py:121-125 */
  MI_BERNOULLI_PROBS = 2,   /* roles: probs, -, value (clamped)   bernoulli.py:104-106, utils.py:101-137 */
  MI_BETA = 3,              /* roles: concentration1, concentration0, value  beta.py:88-92, dirichlet.py:90-97 */
  MI_GAMMA = 4,             /* roles: concentration, rate, value  torch/distributions/gamma.py:90-99 */
  MI_POISSON = 5,           /* roles: rate, -, value              torch/distributions/poisson.py:60-65 */
  MI_INVERSE_GAMMA = 6,     /* roles: concentration, rate, value  mininf/distributions.py:5-11: Gamma
                               through PowerTransform(-1), transformed_distribution.py:151-170 */
  MI_EXPONENTIAL = 7,       /* roles: rate, -, value              torch/distributions/exponential.py:73-76 */
  MI_LAPLACE = 8,           /* roles: loc, scale, value           torch/distributions/laplace.py:88-91 */
  MI_CAUCHY = 9,            /* roles: loc, scale, value           torch/distributions/cauchy.py:82-89 */
  MI_HALF_NORMAL = 10,      /* roles: scale, -, value             half_normal.py:69-74: Normal(0, scale) + log 2 */
  MI_HALF_CAUCHY = 11,      /* roles: scale, -, value             half_cauchy.py:74-82: Cauchy(0, scale) + log 2 */
  MI_LOG_NORMAL = 12,       /* roles: loc, scale, value           log_normal.py:49-55: Normal through
                               ExpTransform, transformed_distribution.py:151-170 */
  MI_STUDENT_T = 13,        /* roles: loc, scale, value; df = mi_site.extra (a constant of the site)
                               torch/distributions/studentT.py:102-113 */
  MI_BINOMIAL = 14,         /* roles: total_count, logits, value  torch/distributions/binomial.py:140-158;
                               no gradient for total_count */
  MI_NEGATIVE_BINOMIAL = 15 /* roles: total_count, logits, value  negative_binomial.py:130-150 */
};

/* what to do with d(site total)/d(operand) */
enum mi_grad_mode {
  MI_GRAD_NONE = 0,
  MI_GRAD_DENSE = 1,     /* write g0 * dT_k/dx[k,i] to `grad` (same logical [K,N] space) */
  MI_GRAD_PARTICLE = 2   /* operand is one scalar per particle: reduce dT_k/dx[k] into slot `slot` */
};

/* flag bits reported per site */
/* mi_group.options: the caller has zeroed `flags` (e.g. one buffer for every group of a step),
 * so mi_group_forward does not reset them. */
#define MI_GROUP_FLAGS_ZEROED 1
/* mi_group.options: leave the fused draw's per-particle-block partial sums of dloc / dscale in the
 * workspace (mi_group_draw_partials) instead of reducing them into draw.dloc / draw.dscale -- the
 * ELBO backward reduces them (MI_DRAW_PARTIALS). */
#define MI_GROUP_DRAW_PARTIALS 2
/* mi_group.options: leave the site values summed over the particles (mi_reduce.ksum) instead of
 * one partial per (segment, particle). Honoured by the Bernoulli BCAST kernel over unmasked
 * contiguous data (k_site_bcast_smem) with at most MI_REDUCE_MAX_SEG segments and K <=
 * MI_KSUM_MAX_K, and ignored by every other launch (reduce->ksum says which was taken). The
 * caller must hand the reduction to mi_elbo_forward: with this option honoured,
 * mi_group_forward_deferred returns MI_EUNSUPPORTED before launching anything when `reduce` is
 * NULL or `site_lp` is not (per-particle values do not exist in this form), and the workspace
 * (mi_group_workspace_bytes) has no [nseg, K] block for the site value. */
#define MI_GROUP_KSUM 4
#define MI_KSUM_MAX_K 8192

#define MI_FLAG_SUPPORT 1u  /* a (non-masked) value lies outside the family's support */
#define MI_FLAG_PARAM 2u    /* a parameter violates its constraint (e.g. scale <= 0) */
#define MI_FLAG_INTERNAL 0x40000000u  /* an in-kernel completion wait gave up (never expected) */

typedef struct mi_operand {
  const float* data;
  int64_t stride_k;
  int64_t stride_i;
  int32_t grad_mode;     /* enum mi_grad_mode */
  int32_t slot;          /* MI_GRAD_PARTICLE: reduction slot in [0, num_slots) */
  float* grad;           /* MI_GRAD_DENSE: output */
  int64_t grad_stride_k;
  int64_t grad_stride_i;
} mi_operand;

typedef struct mi_site {
  int32_t family;        /* enum mi_family */
  int32_t operand[3];    /* role -> operand index, or -1 to use constant[role] */
  float constant[3];
  float extra;           /* a family's fourth, constant input: MI_STUDENT_T's df; unused (0) otherwise.
                            Takes the place of the former padding word: same size and offset */
  const uint8_t* mask;   /* NULL = all observed; else bool bytes, masked-out elements contribute 0 */
  int64_t mask_stride_k;
  int64_t mask_stride_i;
  double scale;          /* minibatch scale: declared batch numel / observed numel (core.py:267-271) */
} mi_site;

/* A guide draw evaluated inside a site group instead of being read from memory: the operand
 * `operand - 1` of the group is z[k, i] = loc[i] + eps[k, i] * scale[i] with eps the counter-based
 * normals of mi_normal_rsample (same seed, step, stream and particle numbering, so the values are
 * bit-identical). The [K, N] draw and its [K, N] gradient never exist in memory: with
 * compute_grads the group writes
 *   dloc[i]   = sum_k g0 * dT_k / dz[k, i]
 *   dscale[i] = sum_k g0 * dT_k / dz[k, i] * eps[k, i]
 * (the gradients mi_normal_rsample_backward would produce from the dense dz). Requirements: the
 * group's other dense operands are row-major [K, N] with unit element stride, N % 4 == 0 and
 * N >= 512; otherwise mi_group_forward returns MI_EUNSUPPORTED and the caller materialises the
 * draw with mi_normal_rsample. */
typedef struct mi_draw {
  int32_t operand;          /* 1 + index of the operand replaced by the draw; 0 = no draw (so a
                               zero-initialised descriptor has none) */
  uint32_t stream_id;
  const float* loc;
  int64_t loc_stride;       /* element strides (0: one value for all elements) */
  const float* scale;
  int64_t scale_stride;
  uint64_t seed;
  uint64_t step;
  const uint64_t* step_device;  /* may be NULL; added to step */
  int64_t particle_offset;
  float* dloc;              /* [N] outputs (compute_grads) */
  float* dscale;
  /* scale_exp non-NULL: the scale is expf(scale_exp[i * scale_stride]) (a guide's
   * transform_to(positive), nn.py:86-96, as mi_transform_params) and the first particle block
   * writes it to `scale` -- the transform inside the draw's kernel */
  const float* scale_exp;
  /* Global index of element 0 of this draw (a multiple of 4; 0 unless the guide factor is sharded
   * over ranks along its elements, mininf_amd.distributed.DataShard): element i uses the
   * counter block of global element element_offset + i, so the ranks' slices draw exactly what
   * one process drawing all elements would. */
  int64_t element_offset;
} mi_draw;

/* Independent work carried by extra workgroups of a group's launch (see mi_group_side_supported):
 * the per-draw Beta implicit-gradient factors of mi_beta_dgrad for draws x [K, N] (row-major) of
 * Beta(c1, c0), written to out [K, N, 2] (fp64). Their fp64 chains are latency-bound and
 * independent of the group's sites, so they run beside the site kernel's VALU-bound workgroups
 * instead of inside mi_elbo_forward (which then reads them through mi_factor.dgrad).
 * out == NULL: no side job (a zero-initialised descriptor has none). */
typedef struct mi_side {
  const float* x;
  const float* c1;
  int64_t c1_stride;
  const float* c0;
  int64_t c0_stride;
  int64_t K;
  int64_t N;
  double* out;
} mi_side;

/* A one-element-per-particle site folded into a group's launch (replaces the prior site's own launch
 * of the README model, README.md:43-47, `sample("theta", Beta(2, 2))`): its value is operand
 * sites[0].operand[0] of the group -- the per-particle parameter of the group's site, e.g. the
 * coin's theta -- its parameters are constants, and its scale is sites[0].scale. Its log-density
 * joins site 0's value, d log p / d value joins that operand's slot gradient, and its validation
 * bits go to *flags. Only the Bernoulli BCAST kernel carries it
 * (mi_group_prior_supported); mi_group_forward returns MI_EUNSUPPORTED otherwise. */
typedef struct mi_prior {
  int32_t present;       /* 0: no folded prior site */
  int32_t family;        /* MI_BETA (c1, c0), MI_NORMAL (loc, scale) or MI_GAMMA (conc., rate) */
  float constant[2];
  double scale;          /* the prior site's scale (a group's: equal to sites[0].scale) */
  uint32_t* flags;       /* the prior site's validation word (MI_FLAG_*) */
} mi_prior;

/* A group of sites evaluated over one shared [K, N] element space in a single pass, so that an
 * operand read by several sites (e.g. a latent z that is the value of one site and the loc of
 * another) is loaded once and its gradient accumulated in registers. */
typedef struct mi_group {
  int64_t K;
  int64_t N;
  int32_t num_sites;
  int32_t num_operands;
  int32_t num_slots;
  int32_t compute_grads; /* 0: forward values only */
  float grad_scale;      /* g0: upstream dL/dT_k assumed for MI_GRAD_DENSE / PARTICLE outputs */
  int32_t options;       /* MI_GROUP_* bits */
  mi_site sites[MI_MAX_SITES];
  mi_operand operands[MI_MAX_OPERANDS];
  mi_draw draw;          /* draw.operand == 0: no operand is a fused guide draw */
  mi_side side;          /* side.out == NULL: no side job */
  mi_prior prior;        /* prior.present == 0: no folded prior site */
  /* pdraw.operand != 0: operand pdraw.operand - 1 is a per-particle operand (stride_i == 0) that is
   * the guide's draw of a one-element Normal factor (the missing-observations model's mu,
   * FactorizedDistribution.rsample, nn.py:133-145): value_k = loc[0] + eps_k * scale[0] with the
   * eps of mi_normal_rsample for (particle_offset + k, element 0; same seed, step, stream --
   * bit-identical), scale = expf(scale_exp[0]) when scale_exp is non-NULL (then also written to
   * scale). The launch computes the values itself and writes them to the operand's data (column
   * block 0) instead of a mi_normal_rsample launch before it. Fused-draw site programs only
   * (mi_group_pdraw_supported; else MI_EUNSUPPORTED: launch mi_normal_rsample first). */
  mi_draw pdraw;
  /* non-NULL: the main site kernel folds its span into stamps[0] (min over workgroups of the start)
   * and stamps[1] (max of the end), on the device's constant-rate clock (mi_wall_clock_khz);
   * initialise them to (UINT64_MAX, 0). Timing only (bench.py); NULL in production launches. */
  unsigned long long* stamps;
} mi_group;

/* Frequency of the clock the span stamps count (mi_group.stamps), in kHz. */
int mi_wall_clock_khz(int* khz);

/* Library identification: returns MI_ABI_VERSION and writes the offload target ("gfx950"). */
int mi_abi_version(char* target, size_t target_bytes);

/* sizeof(mi_operand), sizeof(mi_site), sizeof(mi_group) as compiled: lets bindings check layout. */
int mi_struct_sizes(size_t* operand, size_t* site, size_t* group);

/* ---- site log-probability accumulation (replaces core.py:211-273 + torch log_prob) ------------ */

/* *supported = 1 when mi_group_forward runs `group`'s side job (the Bernoulli BCAST kernel over
 * unmasked contiguous data carries it), else 0: the caller then computes the factors elsewhere. */
int mi_group_side_supported(const mi_group* group, int* supported);

/* *supported = 1 when mi_group_forward evaluates `group`'s folded prior site (mi_prior), else 0:
 * the caller then launches that site on its own. */
int mi_group_prior_supported(const mi_group* group, int* supported);

/* *supported = 1 when mi_group_forward makes `group`'s per-particle draw (mi_group.pdraw). */
int mi_group_pdraw_supported(const mi_group* group, int* supported);

/* Workspace needed by mi_group_forward for this descriptor. */
int mi_group_workspace_bytes(const mi_group* group, size_t* bytes);

/* Evaluate all sites of `group` for every particle:
 *   total[k]              = sum_s scale_s * sum_i mask_si * log p_s(value_ki | params_ki)  (fp32)
 *   site_lp[s*K + k]      = scale_s * sum_i mask_si * log p_s(...)  (fp64; may be NULL)
 *   slot_grad[j*K + k]    = g0 * dT_k / d x[k] for MI_GRAD_PARTICLE operands in slot j (fp32)
 *   operands[o].grad      = g0 * dT_k / d x[k,i] for MI_GRAD_DENSE operands
 *   flags[s]              = OR of MI_FLAG_* found for site s (zeroed by this call unless
 *                           options has MI_GROUP_FLAGS_ZEROED)
 * Replaces LogProbTracer.sample's dist.log_prob (core.py:241, masked branch core.py:231-239),
 * LogProbTracer.total/contribution (core.py:247-273) and the autograd backward of the same ops. */
int mi_group_forward(const mi_group* group, void* workspace, size_t workspace_bytes, float* total,
                     double* site_lp, float* slot_grad, uint32_t* flags, void* stream);

/* ---- deferred finalize reductions --------------------------------------------------------------
 * A site launch ends with a fixed-order fp64 reduction of its per-(segment, particle) partials
 *   part[(v * nseg + seg) * K + k],  v < num_sites: site log densities, then num_slots slot values
 * into total[k] = sum_v scale[v] * sum_seg part (site_lp[v * K + k] the same per site, when
 * non-NULL) and slot_grad[j * K + k] = slot_scale * sum_seg part[num_sites + j]. The *_deferred
 * forms of the site launches skip that reduction when the segment list is at most
 * MI_REDUCE_MAX_SEG long and describe it in *reduce instead (reduce->part == NULL: the launch
 * reduced itself); mi_elbo_forward then runs it (mi_elbo.reduce) in the same launch as the ELBO's
 * own reduction -- one kernel launch less per site launch. The partials live in the site launch's
 * workspace, which must stay untouched until then. mi_reduce_launch runs a described reduction on
 * its own (a caller that cannot hand it to the ELBO). */
#define MI_MAX_REDUCE 4
#define MI_REDUCE_MAX_SEG 1024
typedef struct mi_reduce {
  const float* part;
  int64_t nseg;
  int64_t K;
  int32_t num_sites;
  int32_t num_slots;
  /* bit v: value v's segment block [nseg * K] holds a rank-one sum instead: u[0 .. nseg) at its
   * start, then f[0 .. K) and e[0 .. K); the value is f[k] * sum_seg u[seg] + e[k] (a per-particle
   * constant times a particle-independent sum, e.g. a Bernoulli site's slot gradient over shared
   * data: w dl_k * sum_i x_i - w dl_k N sigmoid(l_k)) */
  int32_t rank1;
  /* 0, or every site value's bit ((1 << num_sites) - 1; anything else is MI_EINVAL). Bit v: value
   * v arrives summed over the particles (MI_GROUP_KSUM). It has
   * no segment block in `part` -- the other values' blocks follow one another without it, value
   * v's block being number v - popcount(ksum & ((1 << v) - 1)) -- and its sum over segments and
   * particles is the fixed-order fp64 sum of nksum doubles, one per site workgroup that evaluated
   * a share. The doubles follow the blocks, [popcount(ksum), nksum] row-major (a value's row: its
   * rank among the set bits) at byte offset round_up(blocks * nseg * K * sizeof(float), 256) of
   * `part`, blocks = num_sites + num_slots - popcount(ksum); `part` is 8-byte aligned.
   * For a job with any bit set, total[k] is NOT written (no per-particle value exists) and
   * site_lp must be NULL: mi_elbo_forward adds g0 * scale[v] * sum straight into the loss.
   * mi_reduce_launch returns MI_EUNSUPPORTED for such a job. */
  int32_t ksum;
  double scale[MI_MAX_SITES];
  double slot_scale;
  float* total;          /* [K] (not written when ksum != 0) */
  double* site_lp;       /* [num_sites, K] or NULL */
  float* slot_grad;      /* [num_slots, K] (num_slots > 0) */
  int64_t nksum;         /* ksum != 0: doubles per particle-summed value */
} mi_reduce;

/* mi_group_forward with the finalize handed to the caller through *reduce (see above). When
 * non-NULL, the hipEvent_t `start_event` / `stop_event` are recorded on `stream` immediately before
 * and after the main site kernel (not the flag reset or the finalize reduction), so the caller can
 * time exactly the roofline-bound kernel of an eager launch. Events are eager-only: while `stream`
 * is capturing, a call with either event returns MI_EUNSUPPORTED before enqueuing anything (the
 * capture stays valid); a replayed kernel is timed by `mi_group.stamps` instead. */
int mi_group_forward_deferred(const mi_group* group, void* workspace, size_t workspace_bytes,
                              float* total, double* site_lp, float* slot_grad, uint32_t* flags,
                              void* start_event, void* stop_event, void* stream, mi_reduce* reduce);

/* Run a deferred reduction as its own launch (MI_EUNSUPPORTED for a job with particle-summed
 * values, mi_reduce.ksum: only mi_elbo_forward finishes those). */
int mi_reduce_launch(const mi_reduce* reduce, void* stream);

/* Where a fused-draw group leaves its partial sums (MI_GROUP_DRAW_PARTIALS): dloc partials are
 * rows [rows, N] at workspace + offset_bytes, dscale partials the next rows * N floats. */
int mi_group_draw_partials(const mi_group* group, size_t* offset_bytes, int64_t* rows);

/* The kernel source the engine specialises for `group` (site families, role kinds and gradient
 * targets compiled in; see mininf_amd/csrc/jit.cpp). Writes at most out_bytes (NUL-terminated) and
 * the full size to *needed. Diagnostic; not on the hot path. */
int mi_group_source(const mi_group* group, char* out, size_t out_bytes, size_t* needed);

/* Compile (hiprtc only; no device needed) the kernel mi_group_source would return. 0 on success,
 * MI_EUNSUPPORTED with the compiler log in `log` otherwise. */
int mi_group_compile_check(const mi_group* group, char* log, size_t log_bytes);

/* Backward rescale of a speculative dense gradient: row k of x is multiplied by g[k] / g0; thread
 * blocks whose rows all have g[k] == g0 return immediately (the common ELBO case). */
int mi_scale_rows(float* x, int64_t stride_k, int64_t stride_i, int64_t K, int64_t N,
                  const float* g, float g0, void* stream);

/* Categorical site (replaces Categorical.__init__'s normalisation, categorical.py:74-78, and
 * log_prob, categorical.py:150-156): logits[k, i, c] raw (or already normalised), value int64:
 *   total[k] = scale * sum_i mask_i * (logits[k, i, value_i] - logsumexp_c logits[k, i, c])
 * and, when dlogits != NULL (same strides as logits), every entry is written:
 *   dlogits[k, i, c] = g0 * scale * mask_i * ([c == value_i] - softmax_c(logits[k, i, :])).
 * A value outside [0, C) of an observed element sets MI_FLAG_SUPPORT in flags[0]. */
int mi_categorical_forward(const float* logits, int64_t stride_k, int64_t stride_i,
                           int64_t stride_c, int64_t K, int64_t N, int64_t C,
                           const int64_t* value, int64_t value_stride_k, int64_t value_stride_i,
                           const uint8_t* mask, int64_t mask_stride_i, double scale, float g0,
                           float* dlogits, void* workspace, size_t workspace_bytes, float* total,
                           uint32_t* flags, void* stream);
int mi_categorical_workspace_bytes(int64_t K, int64_t N, size_t* bytes);

/* Largest number of categories C = event_shape[0] of a Dirichlet the kernels below take (larger:
 * MI_EUNSUPPORTED, checked before any device work). */
#define MI_DIRICHLET_MAX_C 1024

/* Dirichlet site (replaces Dirichlet.log_prob, dirichlet.py:90-97, and its autograd):
 * concentration[k, i, c] and value[k, i, c] by strides (stride_k = 0 for a particle-constant
 * tensor), optional mask[i]:
 *   total[k] = scale * sum_i mask_i * (sum_c xlogy(a_c - 1, x_c) + lgamma(a0) - sum_c lgamma(a_c))
 * with a0 = sum_c a_c in fp32 (as torch), the lgamma terms and every sum in fp64 in a fixed order
 * (no atomics). When non-NULL, dconcentration / dvalue (row-major contiguous [K, N, C]) are
 * written in every entry, zeros on masked rows:
 *   dconcentration[k, i, c] = g0 * scale * (log x_c + psi(a0) - psi(a_c))     (digamma in fp64)
 *   dvalue[k, i, c]         = g0 * scale * (a_c - 1) / x_c
 * following torch's autograd formulas of xlogy at a_c = 1 (no log x_c term where x_c <= 0).
 * flags[0] (zeroed by this call) = MI_FLAG_PARAM if an observed a_c is not > 0, MI_FLAG_SUPPORT
 * unless every observed x_c >= 0 and |sum_c x_c - 1| < 1e-6 (torch's simplex, the sum in fp64).
 * The workspace holds the rows' fp64 log densities. 1 <= C <= MI_DIRICHLET_MAX_C. */
int mi_dirichlet_forward(const float* concentration, int64_t stride_k, int64_t stride_i,
                         int64_t stride_c, int64_t K, int64_t N, int64_t C, const float* value,
                         int64_t value_stride_k, int64_t value_stride_i, int64_t value_stride_c,
                         const uint8_t* mask, int64_t mask_stride_i, double scale, float g0,
                         float* dconcentration, float* dvalue, void* workspace,
                         size_t workspace_bytes, float* total, uint32_t* flags, void* stream);
int mi_dirichlet_workspace_bytes(int64_t K, int64_t N, int64_t C, size_t* bytes);

/* Largest number of components C of a Normal mixture the site kernel below takes (larger:
 * MI_EUNSUPPORTED, checked before any device work). */
#define MI_MIXTURE_MAX_C 1024

/* Normal-mixture site (replaces MixtureSameFamily(Categorical, Normal).log_prob,
 * mixture_same_family.py:169-179, and its autograd): logits[k, i, c], loc[k, i, c] and
 * component_scale[k, i, c] each by its own three strides, any of which may be 0 (a particle-
 * constant tensor, components shared by the rows), value[k, i] by two, optional mask[i]. Per
 * row, with m = log_softmax(logits) taken here (raw and normalised logits both do) and
 * z_c = (x - loc_c) / scale_c:
 *   t_c = m_c - log scale_c - 1/2 log 2 pi - 1/2 z_c^2,  l = logsumexp_c t_c,  r_c = exp(t_c - l)
 *   total[k] = scale * sum_i mask_i * l_ki
 * Both maxima are subtracted before the sums (a value far from every component keeps a finite l);
 * the rows are accumulated in fp64 in a fixed order (no atomics). When non-NULL, dlogits / dloc /
 * dscale (row-major contiguous [K, N, C]) and dvalue ([K, N]) are written in every entry, zeros on
 * masked rows:
 *   dlogits = g0 * scale * (r_c - exp(m_c))         dloc   = g0 * scale * r_c z_c / scale_c
 *   dscale  = g0 * scale * r_c (z_c^2 - 1) / scale_c  dvalue = -g0 * scale * sum_c r_c z_c / scale_c
 * A component of logit -inf has r_c = 0 and zero gradients. flags[0] (zeroed by this call) =
 * MI_FLAG_PARAM unless every observed scale_c > 0 and the row has a finite logit and no NaN logit,
 * MI_FLAG_SUPPORT for a NaN value of an observed row. The workspace holds the rows' fp64 log
 * densities. 1 <= C <= MI_MIXTURE_MAX_C. */
int mi_mixture_normal_forward(const float* logits, int64_t logits_stride_k,
                              int64_t logits_stride_i, int64_t logits_stride_c, const float* loc,
                              int64_t loc_stride_k, int64_t loc_stride_i, int64_t loc_stride_c,
                              const float* component_scale, int64_t scale_stride_k,
                              int64_t scale_stride_i, int64_t scale_stride_c, int64_t K, int64_t N,
                              int64_t C, const float* value, int64_t value_stride_k,
                              int64_t value_stride_i, const uint8_t* mask, int64_t mask_stride_i,
                              double scale, float g0, float* dlogits, float* dloc, float* dscale,
                              float* dvalue, void* workspace, size_t workspace_bytes, float* total,
                              uint32_t* flags, void* stream);
int mi_mixture_normal_workspace_bytes(int64_t K, int64_t N, int64_t C, size_t* bytes);

/* MultivariateNormal site (replaces MultivariateNormal.log_prob, multivariate_normal.py:255-262,
 * with _batch_mahalanobis at :80-102; sites such as examples/missing-observations.md:42), float64,
 * row-major contiguous value[b, n], loc[b, n] and lower-triangular scale_tril[b, n, n] (the
 * caller factorises the covariance). Per batch item b, with w = L^-1 (value - loc):
 *   log_prob[b] = -0.5 w.w - sum_i log L_ii - n/2 log(2 pi),
 * and w[b, :], u[b, :] = L^-T w are written for the gradients:
 *   d/dvalue = -u, d/dloc = u, d/dL = tril(u w^T) - diag(1 / L_ii).
 * n <= MI_MVN_MAX_N. */
#define MI_MVN_MAX_N 1024

/* Cholesky factorisation A = L L^T (replaces torch.linalg.cholesky / cholesky_ex, which
 * MultivariateNormal(loc, covariance_matrix) calls in its constructor, multivariate_normal.py:193,
 * for the GP site of examples/missing-observations.md:40-42): batch row-major [n, n] matrices,
 * float32 or float64 in and out (a_bytes / l_bytes = 4 or 8; n > 80 needs a float64 output),
 * float64 arithmetic. Only the lower triangle of A is read; L's upper triangle is written as 0.
 * info[b] (optional) = 0 or j + 1 for the first non-positive pivot (cholesky_ex's convention).
 * Runs on the caller's stream with no host synchronisation, so a captured graph can hold it
 * (rocSOLVER's potrf cannot be captured on this stack). n <= MI_MVN_MAX_N. */
int mi_cholesky(const void* A, int32_t a_bytes, int64_t batch, int64_t n, void* L,
                int32_t l_bytes, int32_t* info, void* stream);
int mi_mvn_tril_forward(const double* value, const double* loc, const double* scale_tril,
                        int64_t batch, int64_t n, double* log_prob, double* w, double* u,
                        void* stream);

/* ---- guide reparameterised sampling (replaces nn.py:133-145 -> Normal/Beta.rsample) ------------ */

/* Counter-based Philox-4x32-7 normals: eps[k, i] is a function of (seed, step, stream_id,
 * particle_offset + k, element_offset + i) only, so the union of draws is independent of how
 * particles (particle_offset) or elements (element_offset, a multiple of 4) are sharded across
 * GPUs. z[k, i] = loc[i] + eps[k, i] * scale[i] (normal.py:83-86). If `eps` is non-NULL it is
 * used instead of the generator (parity mode: injected host noise, row-major [K, N]).
 * The effective step is `step + *step_device` when `step_device` (a device uint64) is non-NULL, so
 * a captured HIP graph advances the generator by incrementing that word on the device. */
int mi_normal_rsample(const float* loc, int64_t loc_stride, const float* scale, int64_t scale_stride,
                      int64_t K, int64_t N, uint64_t seed, uint64_t step,
                      const uint64_t* step_device, uint32_t stream_id, int64_t particle_offset,
                      int64_t element_offset, const float* eps, float* z, void* stream);

/* mi_normal_rsample for a guide whose scale is exp of an unconstrained parameter u
 * (ParameterizedDistribution.forward, nn.py:86-96 -> transform_to(positive)): the draws use
 * expf(u[i * u_stride]) (as mi_transform_params) and the first particle block writes it to
 * scale_out[i * u_stride] -- the transform and the draw in one launch. */
int mi_normal_rsample_exp(const float* loc, int64_t loc_stride, const float* u, int64_t u_stride,
                          float* scale_out, int64_t K, int64_t N, uint64_t seed, uint64_t step,
                          const uint64_t* step_device, uint32_t stream_id, int64_t particle_offset,
                          int64_t element_offset, const float* eps, float* z, void* stream);

/* Backward of mi_normal_rsample: dloc[i] = sum_k dz[k,i], dscale[i] = sum_k dz[k,i] * eps[k,i]
 * with eps regenerated from the counter (or read from `eps`). */
int mi_normal_rsample_backward_workspace_bytes(int64_t K, int64_t N, size_t* bytes);
int mi_normal_rsample_backward(const float* dz, int64_t dz_stride_k, int64_t dz_stride_i,
                               int64_t K, int64_t N, uint64_t seed, uint64_t step,
                               const uint64_t* step_device, uint32_t stream_id,
                               int64_t particle_offset, int64_t element_offset, const float* eps,
                               void* workspace, size_t workspace_bytes, float* dloc, float* dscale,
                               void* stream);

/* Full-covariance MultivariateNormal guide factor (replaces MultivariateNormal.rsample,
 * multivariate_normal.py:247-250, over K particles): loc[D], row-major contiguous scale_tril[D, D]
 * of which only the lower triangle is read, and
 *   z[k, i] = loc[i] + sum_{j <= i} scale_tril[i, j] * eps[k, j]            (row-major [K, D])
 * with eps[k, j] exactly the normal mi_normal_rsample / mi_philox_normal produce for (seed,
 * step (+ *step_device), stream_id, particle_offset + k, element j) with N = D, or read from `eps`
 * (row-major [K, D]) when it is non-NULL (parity mode). The sum runs over j ascending as one fp32
 * fma chain starting from loc[i], on v_mfma_f32_32x32x2_f32 for D >= 32: row k of a draw with
 * particle_offset = o is bit-identical to row k + o of the draw with particle_offset = 0.
 * 1 <= D <= MI_MVN_MAX_N (larger: MI_EUNSUPPORTED), K >= 1; checked before any device work. */
int mi_mvn_rsample(const float* loc, const float* scale_tril, int64_t K, int64_t D,
                   uint64_t seed, uint64_t step, const uint64_t* step_device, uint32_t stream_id,
                   int64_t particle_offset, const float* eps, float* z, void* stream);

/* Backward of mi_mvn_rsample for upstream dz[k, i] (strided), reduced over particles in a fixed
 * order (no atomics; particle slices are combined in fp64 through the workspace):
 *   dloc[i]           = sum_k dz[k, i]
 *   dscale_tril[i, j] = sum_k dz[k, i] * eps[k, j]   (j <= i), 0 (j > i): all D * D entries written
 * with eps regenerated from the counter (or read from `eps`); the forward never stores it. */
int mi_mvn_rsample_backward_workspace_bytes(int64_t K, int64_t D, size_t* bytes);
int mi_mvn_rsample_backward(const float* dz, int64_t dz_stride_k, int64_t dz_stride_i,
                            int64_t K, int64_t D, uint64_t seed, uint64_t step,
                            const uint64_t* step_device, uint32_t stream_id,
                            int64_t particle_offset, const float* eps,
                            void* workspace, size_t workspace_bytes,
                            float* dloc, float* dscale_tril, void* stream);

/* LowRankMultivariateNormal guide factor (replaces LowRankMultivariateNormal.rsample, torch 2.10
 * lowrank_multivariate_normal.py:214-223, over K particles): loc[D], row-major contiguous
 * cov_factor[D, R], cov_diag[D] > 0, covariance cov_factor cov_factor^T + diag(cov_diag), and
 *   z[k, i] = loc[i] + sum_r cov_factor[i, r] * eps_W[k, r] + sqrt(cov_diag[i]) * eps_D[k, i]
 * (row-major [K, D]). Both sets of normals come from the factor's one Normal stream (seed,
 * step (+ *step_device), stream_id, particle_offset + k): eps_D[k, i] is element i, exactly what
 * mi_normal_rsample / mi_philox_normal produce for it, and eps_W[k, r] is element Dpad + r with
 * Dpad = 4 * ceil(D / 4) (both parts start on a Philox quad). A non-NULL `eps` is read instead
 * (parity mode): row-major [K, D + R], the D columns of eps_D first, then the R of eps_W.
 * Each z[k, i] is one fp32 chain: acc = loc[i]; acc = fma(eps_W[k, r], cov_factor[i, r], acc) for
 * r ascending (on v_mfma_f32_32x32x2_f32 for R >= 32, zero-padded to whole tiles of r);
 * acc = fma(sqrtf(cov_diag[i]), eps_D[k, i], acc) with a correctly rounded square root. Row k of a
 * draw with particle_offset = o is bit-identical to row k + o of the draw with particle_offset = 0,
 * for any K. 1 <= R <= MI_LOWRANK_MAX_R, 1 <= D <= MI_LOWRANK_MAX_D (larger: MI_EUNSUPPORTED),
 * K >= 1; checked before any device work. */
#define MI_LOWRANK_MAX_R 128
#define MI_LOWRANK_MAX_D (1 << 24)
int mi_lowrank_rsample(const float* loc, const float* cov_factor, const float* cov_diag,
                       int64_t K, int64_t D, int64_t R, uint64_t seed, uint64_t step,
                       const uint64_t* step_device, uint32_t stream_id, int64_t particle_offset,
                       const float* eps, float* z, void* stream);

/* Backward of mi_lowrank_rsample for upstream dz[k, i] (strided), reduced over particles in a
 * fixed order (no atomics; particle slices are combined in fp64 through the workspace):
 *   dloc[i]           = sum_k dz[k, i]
 *   dcov_factor[i, r] = sum_k dz[k, i] * eps_W[k, r]
 *   dcov_diag[i]      = (sum_k dz[k, i] * eps_D[k, i]) * 0.5 / sqrt(cov_diag[i])
 * with the normals regenerated from the counter (or read from `eps`); the forward stores none. */
int mi_lowrank_rsample_backward_workspace_bytes(int64_t K, int64_t D, int64_t R, size_t* bytes);
int mi_lowrank_rsample_backward(const float* dz, int64_t dz_stride_k, int64_t dz_stride_i,
                                const float* cov_diag, int64_t K, int64_t D, int64_t R,
                                uint64_t seed, uint64_t step, const uint64_t* step_device,
                                uint32_t stream_id, int64_t particle_offset, const float* eps,
                                void* workspace, size_t workspace_bytes, float* dloc,
                                float* dcov_factor, float* dcov_diag, void* stream);

/* Entropy of the same factor (replaces LowRankMultivariateNormal.entropy, torch 2.10
 * lowrank_multivariate_normal.py:225-237) and its gradient in closed form, from row-major
 * contiguous W = cov_factor[D, R], d = cov_diag[D] and L = capacitance_tril[R, R], the lower
 * Cholesky factor of C = I + W^T diag(1 / d) W that the constructor keeps as _capacitance_tril
 * (only its lower triangle is read). With M = W C^-1:
 *   entropy           = 0.5 D (1 + log 2 pi) + sum_j log L[j, j] + 0.5 sum_i log d[i]
 *   dcov_factor[i, r] = M[i, r] / d[i]
 *   dcov_diag[i]      = 0.5 (1 / d[i] - (sum_r M[i, r] W[i, r]) / d[i]^2)
 * the whole derivative with respect to W and d, L's dependence on them included: nothing is to be
 * propagated through L. Three launches: L^-1 and C^-1 in fp64 by one workgroup (C^-1 handed on as
 * f32), one pass over W (on v_mfma_f32_32x32x2_f32 for R >= 32; W read once, dcov_factor written
 * once), and the log sums combined in fp64 in a fixed order (no atomics: two calls on the same
 * inputs are bit-identical). dcov_factor and dcov_diag may both be NULL: only the value is
 * computed, bit-identical to the one computed with them. The caps are the draw's (beyond them:
 * MI_EUNSUPPORTED); D < 1, R < 1, a NULL required pointer, one gradient pointer without the other
 * or a workspace smaller than mi_lowrank_entropy_workspace_bytes asks for: MI_EINVAL. All checked
 * before any device work. */
int mi_lowrank_entropy_workspace_bytes(int64_t D, int64_t R, size_t* bytes);
int mi_lowrank_entropy(const float* cov_factor, const float* cov_diag,
                       const float* capacitance_tril, int64_t D, int64_t R,
                       void* workspace, size_t workspace_bytes,
                       float* entropy, float* dcov_factor, float* dcov_diag, void* stream);

/* LowRankMultivariateNormal site density (replaces LowRankMultivariateNormal.log_prob, torch 2.10
 * lowrank_multivariate_normal.py:203-212) for K particles and N rows, and its gradients in closed
 * form. All float32; every parameter is read through a particle stride, which may be 0:
 *   value[k, i, :]  at value + k value_stride_k + i value_stride_i, the last axis contiguous
 *                   (value_stride_k = 0: observed data the particles share),
 *   loc[k, :], W = cov_factor[k][D, R] row-major, d = cov_diag[k, :] > 0 and
 *   L = capacitance_tril[k][R, R], the lower Cholesky factor of C = I + W^T diag(1 / d) W that the
 *   constructor keeps as _capacitance_tril (only its lower triangle is read).
 * Forward, per (k, i), with r = x_i - loc, y = r / d, t = W^T y and c = C^-1 t:
 *   log_prob[k, i] = -1/2 (D log 2 pi + 2 sum_j log L[j, j] + sum_j log d[j] + r.y - t.c)
 *   coef[k, i, :]  = c                                       ([K, N] and [K, N, R], contiguous)
 * B = L^-1 is formed per particle in fp64 and handed on as f32, and c = B^T (B t), t.c = |B t|^2:
 * C^-1 itself is never formed (for R > D its product with t loses to rounding what r - W c then
 * cancels against). Both log sums are fp64, and T = Y W is one pass over the rows (on
 * v_mfma_f32_32x32x2_f32 for R >= 32, zero-padded to whole tiles; on the vector pipe below that).
 * Two launches.
 * Backward, for the upstream g[k, i] at g + k g_stride_k + i g_stride_i and the forward's coef, with
 * a_i = (r_i - W c_i) / d, G_k = sum_i g[k, i] and M = W C^-1:
 *   dvalue[k, i, :]   = -g_i a_i                                             [K, N, D]
 *   dloc[k, :]        = sum_i g_i a_i                                        [K, D]
 *   dcov_factor[k]    = sum_i g_i a_i c_i^T - G_k M / d[:, None]             [K, D, R]
 *   dcov_diag[k, j]   = 1/2 sum_i g_i a_ij^2
 *                       - 1/2 G_k (1 / d_j - (sum_r M[j, r] W[j, r]) / d_j^2) [K, D]
 * (contiguous) -- the whole derivatives with respect to W and d, L's dependence on them included:
 * nothing is to be propagated into capacitance_tril. Each of the four may be NULL and is then not
 * computed; the others are bit-identical to those of the call that asks for all four. A row with
 * g_i == 0 contributes exact zeros everywhere, whatever its value holds (NaN included). The row
 * sums have a fixed order: per-slice partials in the workspace, each a chain in row order, summed
 * in slice order by a finishing launch (no atomics: two calls on the same inputs are
 * bit-identical). 1 <= R <= MI_LOWRANK_MAX_R, 1 <= D <= MI_LOWRANK_SITE_MAX_D and K * D and
 * K * ceil(N / 32) within a grid's 2^31 - 1 blocks (beyond: MI_EUNSUPPORTED); K, N, D or R < 1, a NULL
 * required pointer or a workspace smaller than mi_lowrank_site_workspace_bytes asks for (one size
 * serves both calls): MI_EINVAL. All checked before any device work. */
#define MI_LOWRANK_SITE_MAX_D (1 << 16)
int mi_lowrank_site_workspace_bytes(int64_t K, int64_t N, int64_t D, int64_t R, size_t* bytes);
int mi_lowrank_site_forward(const float* value, int64_t value_stride_k, int64_t value_stride_i,
                            const float* loc, int64_t loc_stride_k,
                            const float* cov_factor, int64_t cov_factor_stride_k,
                            const float* cov_diag, int64_t cov_diag_stride_k,
                            const float* capacitance_tril, int64_t capacitance_tril_stride_k,
                            int64_t K, int64_t N, int64_t D, int64_t R,
                            void* workspace, size_t workspace_bytes,
                            float* log_prob, float* coef, void* stream);
int mi_lowrank_site_backward(const float* g, int64_t g_stride_k, int64_t g_stride_i,
                             const float* value, int64_t value_stride_k, int64_t value_stride_i,
                             const float* loc, int64_t loc_stride_k,
                             const float* cov_factor, int64_t cov_factor_stride_k,
                             const float* cov_diag, int64_t cov_diag_stride_k,
                             const float* capacitance_tril, int64_t capacitance_tril_stride_k,
                             const float* coef, int64_t K, int64_t N, int64_t D, int64_t R,
                             void* workspace, size_t workspace_bytes,
                             float* dvalue, float* dloc, float* dcov_factor, float* dcov_diag,
                             void* stream);

/* Beta(concentration1, concentration0) draws x[k, i] = G1 / (G1 + G0) with Marsaglia-Tsang gamma
 * variates from the same counter-based generator (beta.py:85-86, dirichlet.py:23-36, 85-88). With
 * `x_in` non-NULL the draws are copied from it instead (parity mode). */
int mi_beta_rsample(const float* c1, int64_t c1_stride, const float* c0, int64_t c0_stride,
                    int64_t K, int64_t N, uint64_t seed, uint64_t step,
                    const uint64_t* step_device, uint32_t stream_id,
                    int64_t particle_offset, const float* x_in, float* x, void* stream);

/* mi_beta_rsample for a guide whose concentrations are exp of unconstrained parameters
 * (ParameterizedDistribution.forward, nn.py:86-96 -> transform_to(positive), and Beta.__init__'s
 * stack, beta.py:36-40): every draw computes its concentrations from u1 / u0 (expf, as
 * mi_transform_params) and the k = 0 draws also write them, interleaved, to conc[N, 2] -- the
 * transform and the draw in one launch. */
int mi_beta_rsample_exp(const float* u1, int64_t u1_stride, const float* u0, int64_t u0_stride,
                        float* conc, int64_t K, int64_t N, uint64_t seed, uint64_t step,
                        const uint64_t* step_device, uint32_t stream_id, int64_t particle_offset,
                        const float* x_in, float* x, void* stream);

/* Implicit reparameterisation gradient of the Beta draws (dirichlet.py:17-20 ->
 * torch._dirichlet_grad, ATen/native/Distributions.h dirichlet_grad_one), reduced over particles:
 *   dc1[i * dc1_stride] = sum_k dx[k,i] * dgrad(x, c1, c1+c0) * (1 - x)
 *   dc0[i * dc0_stride] = -sum_k dx[k,i] * dgrad(1 - x, c0, c1+c0) * x
 * (output strides let the gradient land directly in the interleaved [..., 2] concentration layout
 * torch's Beta keeps, beta.py:36-40). */
int mi_beta_rsample_backward_workspace_bytes(int64_t K, int64_t N, size_t* bytes);
int mi_beta_rsample_backward(const float* dx, int64_t dx_stride_k, int64_t dx_stride_i,
                             const float* x, const float* c1, int64_t c1_stride, const float* c0,
                             int64_t c0_stride, int64_t K, int64_t N, void* workspace,
                             size_t workspace_bytes, float* dc1, int64_t dc1_stride, float* dc0,
                             int64_t dc0_stride, void* stream);

/* The upstream-independent factors of mi_beta_rsample_backward, per draw:
 *   out[(k * N + i) * 2 + 0] =  dgrad(x, c1, c1+c0) * (1 - x)
 *   out[(k * N + i) * 2 + 1] = -dgrad(1 - x, c0, c1+c0) * x          (fp64, [K, N, 2])
 * so dc1[i] = sum_k dx[k,i] * out[k,i,0] and dc0[i] = sum_k dx[k,i] * out[k,i,1]. They depend only
 * on the draws, so this can run beside the site kernels; mi_elbo_forward reads them through
 * mi_factor.dgrad. */
int mi_beta_dgrad(const float* x, const float* c1, int64_t c1_stride, const float* c0,
                  int64_t c0_stride, int64_t K, int64_t N, double* out, void* stream);

/* Recovery after a failed hipGraph capture of a training step (mininf_amd.graph.StepGraph): if
 * `stream` is still capturing, end the capture and destroy the partial graph; then clear the
 * thread's last HIP error. *was_capturing (optional) reports whether a capture had to be ended.
 * The host-side counterpart of the reference's exception semantics: an error raised inside a step
 * (mininf/core.py:142-189, nn.py:212-228) leaves the process usable. Not asynchronous: it acts on
 * the stream's capture state, not on its work. */
int mi_capture_abandon(void* stream, int* was_capturing);

/* Start of one ELBO step (EvidenceLowerBoundLoss.forward) in one launch: *snapshot = *counter (the
 * generator step this call's draws and their backward use), *counter += 1, and
 * flags[0 .. nflags) = 0 (the call's validation words, MI_GROUP_FLAGS_ZEROED). */
int mi_step_begin(uint64_t* counter, uint64_t* snapshot, uint32_t* flags, int64_t nflags,
                  void* stream);

/* Gamma(concentration, rate) guide draws (replaces Gamma.rsample, gamma.py:80-88):
 *   g[k, i] = standard Gamma(concentration[i]) draw (Marsaglia-Tsang, same counter scheme as
 *             mi_beta_rsample, sub-stream 2), or g_in[k, i] when g_in != NULL (parity mode);
 *   x[k, i] = max(g[k, i] / rate[i], FLT_MIN).
 * g is the backward's input (torch saves _standard_gamma's result the same way). */
int mi_gamma_rsample(const float* concentration, int64_t concentration_stride, const float* rate,
                     int64_t rate_stride, int64_t K, int64_t N, uint64_t seed, uint64_t step,
                     const uint64_t* step_device, uint32_t stream_id, int64_t particle_offset,
                     const float* g_in, float* g, float* x, void* stream);
/* Backward for upstream dx[k, i] (strided), reduced over particles in fp64:
 *   dconcentration[i] = sum_k dx / rate * standard_gamma_grad(concentration, g)
 *                       (torch _standard_gamma_grad, Distributions.h:310, in double)
 *   drate[i]          = sum_k -dx * g / rate^2 */
int mi_gamma_rsample_backward_workspace_bytes(int64_t K, int64_t N, size_t* bytes);
int mi_gamma_rsample_backward(const float* dx, int64_t dx_stride_k, int64_t dx_stride_i,
                              const float* g, const float* concentration,
                              int64_t concentration_stride, const float* rate,
                              int64_t rate_stride, int64_t K, int64_t N, void* workspace,
                              size_t workspace_bytes, float* dconcentration,
                              int64_t dconcentration_stride, float* drate, int64_t drate_stride,
                              void* stream);

/* Dirichlet(concentration[N, C], row-major contiguous) guide draws (replaces Dirichlet.rsample,
 * dirichlet.py:85-88 -> torch._sample_dirichlet):
 *   x[k, n, c] = g[k, n, c] / sum_j g[k, n, j]                     (row-major contiguous [K, N, C])
 * with g[k, n, c] exactly the standard Gamma variate mi_gamma_rsample draws for (seed, step
 * (+ *step_device), stream_id, particle_offset + k, element n * C + c) from concentration viewed
 * as [N * C], or g_in[k, n, c] when g_in != NULL (parity mode). The row sum is taken in fp64 in a
 * fixed order and each component divided once, then clamped to [FLT_MIN, 1 - 2^-24] as torch does;
 * a row whose variates all underflow is the (clamped) one-hot of its largest concentration. Row k
 * of a draw with particle_offset = o is bit-identical to row k + o of the draw with offset 0.
 * 1 <= C <= MI_DIRICHLET_MAX_C. */
int mi_dirichlet_rsample(const float* concentration, int64_t K, int64_t N, int64_t C,
                         uint64_t seed, uint64_t step, const uint64_t* step_device,
                         uint32_t stream_id, int64_t particle_offset, const float* g_in, float* x,
                         void* stream);
/* Backward for upstream dx[k, n, c] (strided) and the saved draws x (dirichlet.py:17-20,
 * _Dirichlet_backward), fp64, reduced over particles in a fixed order (no atomics; particle slices
 * are combined through the workspace):
 *   dconcentration[n, c] = sum_k dgrad(x_kc, a_c, a0) * (dx_kc - sum_j x_kj * dx_kj)
 * with dgrad torch._dirichlet_grad (ATen/native/Distributions.h dirichlet_grad_one) and a0 the
 * fp32 row sum of the concentrations. */
int mi_dirichlet_rsample_backward_workspace_bytes(int64_t K, int64_t N, int64_t C, size_t* bytes);
int mi_dirichlet_rsample_backward(const float* dx, int64_t dx_stride_k, int64_t dx_stride_i,
                                  int64_t dx_stride_c, const float* x, const float* concentration,
                                  int64_t K, int64_t N, int64_t C, void* workspace,
                                  size_t workspace_bytes, float* dconcentration, void* stream);

/* Dirichlet entropy (dirichlet.py:122-130) of concentration[N, C] (row-major contiguous), summed
 * over the rows, and its gradient, in one launch, fp64, fixed order:
 *   entropy[0] = sum_n [sum_c lgamma(a_c) - lgamma(a0) - (C - a0) psi(a0) - sum_c (a_c - 1) psi(a_c)]
 *   dconcentration[n, c] = (a0 - C) psi'(a0) - (a_c - 1) psi'(a_c)        (when non-NULL)
 * 1 <= C <= MI_DIRICHLET_MAX_C. */
int mi_dirichlet_entropy(const float* concentration, int64_t N, int64_t C, float* entropy,
                         float* dconcentration, void* stream);

/* Constrained parameters of one guide factor in one launch, interleaved [n, m]:
 *   out[i * m + j] = exp(u[j][i * stride[j]])   (transform[j] MI_TRANSFORM_EXP: transform_to(positive),
 *                                                 torch constraint_registry.py:184-189)
 *                  = u[j][i * stride[j]]        (MI_TRANSFORM_NONE)
 * ParameterizedDistribution.forward (reference nn.py:86-96) for a Beta guide, whose Dirichlet keeps
 * exactly this [..., 2] (concentration1, concentration0) layout (beta.py:36-40). */
#define MI_MAX_PARAMS 4
typedef struct mi_params {
  int32_t m;
  int32_t pad0;
  int64_t n;
  const float* u[MI_MAX_PARAMS];
  int64_t stride[MI_MAX_PARAMS];
  int32_t transform[MI_MAX_PARAMS];
} mi_params;
int mi_transform_params(const mi_params* params, float* out, void* stream);

/* Raw generator output for tests: out[k, i] = standard normal eps of mi_normal_rsample. */
int mi_philox_normal(int64_t K, int64_t N, uint64_t seed, uint64_t step, uint32_t stream_id,
                     int64_t particle_offset, float* out, void* stream);
/* Raw Philox-4x32-10 blocks for known-answer tests: out[4*j .. 4*j+3] = philox(ctr[j], key). */
int mi_philox4x32(const uint32_t* ctr, int64_t count, uint32_t key0, uint32_t key1, uint32_t* out,
                  void* stream);

/* ---- posterior-predictive draws (broadcast_samples, reference core.py:548-584) ---------------- */

/* Draws of the sites a predictive run simulates (SampleTracer.sample, core.py:192-204), on the
 * guide generator. The logical space is [S, M]: S samples of M elements, flat element
 * e = s * M + j, which is mi_normal_rsample's layout with K = 1 and N = S * M. A parameter is a
 * device pointer and two element strides (stride_s, stride_j), either of which may be 0, so a
 * per-sample scalar, a per-element constant and a dense parameter are read in place. A value is a
 * function of (seed, stream_id, s, j, M): not of S, so the first S' samples of a run are the run
 * with S = S'. All three are asynchronous on `stream`, allocate nothing, index in int64 and check
 * their arguments before any device work. */

/* Fixed-consumption families. Element e takes word e % 4 of the Philox block of quad e / 4 at step
 * 0, sub-stream 0, particle 0 (mi_normal_rsample's counter): u = ((word >> 8) + 0.5) * 2^-24, or,
 * for the two normal-based families, the standard normal eps mi_philox_normal reports for e.
 *   MI_PRED_BERNOULLI_PROBS   a = probs           u < a ? 1 : 0
 *   MI_PRED_BERNOULLI_LOGITS  a = logits          u < 1 / (1 + expf(-a)) ? 1 : 0
 *   MI_PRED_EXPONENTIAL       a = rate            -logf(u) / a
 *   MI_PRED_LAPLACE           a = loc, b = scale  a - b * sign(u - 1/2) * log1pf(-2 |u - 1/2|)
 *   MI_PRED_CAUCHY            a = loc, b = scale  a + b * tan(pi (u - 1/2))
 *   MI_PRED_HALF_CAUCHY       a = scale           a * tan(pi u / 2)
 *   MI_PRED_HALF_NORMAL       a = scale           a * |eps|
 *   MI_PRED_LOG_NORMAL        a = loc, b = scale  expf(a + eps * b)
 * u lies on the 24-bit grid (k + 1/2) 2^-24 rounded to float32, so every tail stops at the 2^-25
 * quantile: an Exponential draw is at most 17.33 / rate, a Cauchy draw at least
 * loc - scale * 2^25 / pi, |eps| at most 5.89. Above 1/2 the float32 spacing is 2^-24 and the top
 * grid point rounds to 1.0f; Laplace, Cauchy and HalfCauchy, for which u = 1 is a pole, read it as
 * 1 - 2^-24, so their upper tail stops at the 2^-24 quantile (Cauchy: loc + scale * 2^24 / pi).
 * b is read only by the two-parameter families (NULL otherwise). out is float32 [S * M].
 * S * M <= 2^34 (the quad counter has 32 bits): larger is MI_EUNSUPPORTED. */
#define MI_PRED_BERNOULLI_PROBS 0
#define MI_PRED_BERNOULLI_LOGITS 1
#define MI_PRED_EXPONENTIAL 2
#define MI_PRED_LAPLACE 3
#define MI_PRED_CAUCHY 4
#define MI_PRED_HALF_CAUCHY 5
#define MI_PRED_HALF_NORMAL 6
#define MI_PRED_LOG_NORMAL 7
#define MI_PRED_FAMILIES 8
int mi_predictive_sample(int family, const float* a, int64_t a_stride_s, int64_t a_stride_j,
                         const float* b, int64_t b_stride_s, int64_t b_stride_j, int64_t S,
                         int64_t M, uint64_t seed, uint32_t stream_id, float* out, void* stream);

/* Categorical(logits[S, B, C]) with T replications per sample (the site's sample_shape): row
 * r = (s * T + t) * B + b reads logits[s * stride_s + b * stride_b + c * stride_c] (stride_s or
 * stride_b may be 0) and takes word r % 4 of the block of quad r / 4 (the counter above, over rows).
 *   out[r] = the smallest c with cum_c > u * cum_{C-1},  cum_c = sum_{j <= c} expf(l_j - max_j l_j)
 * accumulated ascending in fp32 (rows of more than 32 categories: per-lane runs of consecutive
 * categories joined by a wave prefix sum, which moves cum_c by rounding only). If rounding lets the
 * search run off the end, out[r] is the last category with a finite logit. out is int64 [S*T*B].
 * 1 <= C <= MI_PRED_CATEGORICAL_MAX_C and S * T * B <= 2^34: larger is MI_EUNSUPPORTED. */
#define MI_PRED_CATEGORICAL_MAX_C 1024
int mi_predictive_categorical(const float* logits, int64_t stride_s, int64_t stride_b,
                              int64_t stride_c, int64_t S, int64_t T, int64_t B, int64_t C,
                              uint64_t seed, uint32_t stream_id, int64_t* out, void* stream);

/* MixtureSameFamily(Categorical(logits[S, B, C]), Normal(loc[S, B, C], scale[S, B, C])) with T
 * replications per sample: row r = (s * T + t) * B + b as above, logits, loc and scale each read
 * through its own (stride_s, stride_b, stride_c). The component c is mi_predictive_categorical's
 * choice for the same seed, stream and logits (sub-stream 0); eps is Box-Muller output r % 4 of the
 * block of quad r / 4 on sub-stream 1 (counter {r / 4, 0, 0, (stream_id << 8) | 1}):
 *   out[r] = loc_c + scale_c * eps.
 * out is float32 [S*T*B]. The caps are mi_predictive_categorical's. */
int mi_predictive_mixture_normal(const float* logits, int64_t logits_stride_s,
                                 int64_t logits_stride_b, int64_t logits_stride_c,
                                 const float* loc, int64_t loc_stride_s, int64_t loc_stride_b,
                                 int64_t loc_stride_c, const float* scale, int64_t scale_stride_s,
                                 int64_t scale_stride_b, int64_t scale_stride_c, int64_t S,
                                 int64_t T, int64_t B, int64_t C, uint64_t seed,
                                 uint32_t stream_id, float* out, void* stream);

/* Poisson(rate) consumes a variable number of words, so element e reads its own stream of Philox
 * blocks, mi_gamma_rsample's scheme on the free sub-stream 3:
 *   counter {e, 0, 0, (stream_id << 8) | (3 << 6) | block}, four words per block.
 * rate < 10: uniforms are multiplied until the product falls below expf(-rate) (fp32; at most 250
 * factors). rate >= 10: Hoermann's transformed rejection PTRS (1993) in fp64, two uniforms per
 * attempt, at most 64 attempts. rate = 0 gives 0; a negative or non-finite rate writes NaN. out
 * is float32 [S * M]. S * M <= 2^32 (the element counter has 32 bits): larger is MI_EUNSUPPORTED. */
int mi_predictive_poisson(const float* rate, int64_t stride_s, int64_t stride_j, int64_t S,
                          int64_t M, uint64_t seed, uint32_t stream_id, float* out, void* stream);

/* ---- guide factors of the one-noise-word families --------------------------------------------- */

/* Exponential, Laplace, Cauchy, HalfCauchy, HalfNormal and LogNormal as guide factors: the draw of
 * mi_predictive_sample's table above over K particles, its backward and the entropy. `family` is
 * MI_PRED_EXPONENTIAL .. MI_PRED_LOG_NORMAL (the two Bernoulli codes are MI_EINVAL); a and b are
 * that table's parameters, each read at i * stride (stride 0: one value for all elements); b is
 * read only by the two-parameter families (NULL otherwise). All are asynchronous on `stream`,
 * allocate nothing, index in int64 and check their arguments before any device work.
 *
 *   z[k, i] = draw(a[i * a_stride], b[i * b_stride], v[k, i])            (row-major [K, N])
 * v[k, i] comes from word i % 4 of the Philox block of counter
 *   {quad i / 4, particle_offset + k, step (+ *step_device), stream_id << 8}
 * which is mi_normal_rsample's counter: u = ((word >> 8) + 0.5) * 2^-24 for the four uniform
 * families, the eps mi_philox_normal reports for HalfNormal and LogNormal. Row k at
 * particle_offset o is row k + o at offset 0. One difference from the predictive draw: here the
 * Exponential too reads u = 1.0f (the top grid point) as 1 - 2^-24, so no draw is 0 and every draw
 * lies inside its family's support. A non-NULL `noise` (row-major [K, N]) is read for v instead
 * (parity mode: neither seed nor step is read). N <= 2^34 and K * ceil(N / 4) <= 2^39: larger is
 * MI_EUNSUPPORTED. */
int mi_elementwise_rsample(int family, const float* a, int64_t a_stride, const float* b,
                           int64_t b_stride, int64_t K, int64_t N, uint64_t seed, uint64_t step,
                           const uint64_t* step_device, uint32_t stream_id,
                           int64_t particle_offset, const float* noise, float* z, void* stream);

/* Backward of the draw, reduced over particles; v is regenerated from the counter (or read from
 * `noise`), z is not needed:
 *   da[i] = sum_k dz[k * dz_stride_k + i * dz_stride_i] * d z / d a,   db[i] likewise
 * each written (contiguous [N]) only when its pointer is non-NULL; at least one must be. db is
 * ignored for the one-parameter families. With t the standardised draw (loc 0, scale 1):
 *   LogNormal   d/dloc = z, d/dscale = z * eps      Laplace, Cauchy  d/dloc = 1, d/dscale = t
 *   HalfCauchy, HalfNormal  d/dscale = t            Exponential      d/drate = logf(u) / rate^2
 * Products and sums are fp64, in an order fixed by (K, N): particle slices write fp32 partials to
 * the workspace and a second launch adds them in slice order; one slice writes the outputs
 * directly. */
int mi_elementwise_rsample_backward_workspace_bytes(int64_t K, int64_t N, size_t* bytes);
int mi_elementwise_rsample_backward(int family, const float* dz, int64_t dz_stride_k,
                                    int64_t dz_stride_i, const float* a, int64_t a_stride,
                                    const float* b, int64_t b_stride, int64_t K, int64_t N,
                                    uint64_t seed, uint64_t step, const uint64_t* step_device,
                                    uint32_t stream_id, int64_t particle_offset,
                                    const float* noise, void* workspace, size_t workspace_bytes,
                                    float* da, float* db, void* stream);

/* Entropy of the factor summed over its N elements, and its gradient, in one launch: H[0] is the
 * fp64 sum (fixed order) of the elements' fp32 entropies, written as one float32; da[i] and db[i]
 * (float32, contiguous [N]) are written only when non-NULL. Per element, torch's entropy() of each
 * class:
 *   LogNormal    1/2 + 1/2 log(2 pi) + log(scale) + loc    dloc = 1, dscale = 1 / scale
 *   Laplace      1 + log(2 scale)                          dloc = 0, dscale = 1 / scale
 *   Cauchy       log(4 pi scale)                           dloc = 0, dscale = 1 / scale
 *   HalfCauchy   log(2 pi scale)                           dscale = 1 / scale
 *   HalfNormal   1/2 + 1/2 log(pi / 2) + log(scale)        dscale = 1 / scale
 *   Exponential  1 - log(rate)                             drate = -1 / rate */
int mi_elementwise_entropy(int family, const float* a, int64_t a_stride, const float* b,
                           int64_t b_stride, int64_t N, float* H, float* da, float* db,
                           void* stream);

/* ---- linear-predictor sites (Normal / Bernoulli-logits / Poisson-log / Binomial / NegativeBinomial
 *      on X @ theta) ---------------------------------------------------------------------------- */

/* A site whose location / logits is the model's own product X @ theta of an observed design matrix
 * X [N, P] and a per-particle coefficient vector theta [K, P] (the reference's regression models:
 * tests/test_mininf.py:13-18, examples/minibatch.md:24-33). The product is evaluated inside the
 * site kernel, so the [K, N] predictor and its gradient never exist in memory:
 *   total[k]        = site_scale * sum_i mask_i * log p(value_i | (X theta_k)_i, sigma_k)
 *   dslots[j*K + k] = g0 * d total[k] / d theta[k, j]   for j < P (slot-major: row j holds all k)
 *   dslots[P*K + k] = g0 * d total[k] / d sigma_k       (Normal with per-particle sigma only)
 *   flags[0]        = OR of MI_FLAG_* (value support; sigma > 0; finite predictor)
 * family: MI_NORMAL (sigma = scale[k * scale_stride_k], or scale_constant when scale == NULL),
 * MI_BERNOULLI_LOGITS (scale unused), or one of the count regressions on eta = (X theta_k)_i
 * (scale unused, no slot past the P of theta):
 *   MI_POISSON            log link, rate = exp(eta):  y eta - exp(eta) - lgamma(y + 1),
 *                         d/d eta = y - exp(eta); y a non-negative integer
 *   MI_BINOMIAL           total_count n_i = count, logits = eta (binomial.py:140-158),
 *                         d/d eta = y - n_i sigmoid(eta); y an integer in [0, n_i]
 *   MI_NEGATIVE_BINOMIAL  total_count r_i = count, logits = eta (negative_binomial.py:130-150,
 *                         with its point mass where r_i + y == 0),
 *                         d/d eta = y - (y + r_i) sigmoid(eta); y a non-negative integer
 * The terms of a row alone (lgamma(y + 1), the binomial coefficient, NegativeBinomial's
 * normalisation) are evaluated once per row and added once per particle. MI_FLAG_SUPPORT: y of an
 * unmasked row outside the support; MI_FLAG_PARAM: a non-finite eta, or on an unmasked row a
 * negative r_i or a negative or non-integer n_i. The Poisson site is evaluated on eta itself: a
 * finite eta whose exp overflows float32 follows IEEE (total = -inf, as torch's Poisson(exp(eta)),
 * no flag), one whose exp underflows keeps y eta finite. P <= MI_LINEAR_MAX_P. */
#define MI_LINEAR_MAX_P 64
/* options bit: run the VALU kernel even where the matrix-core (v_mfma_f32_32x32x2_f32) kernel
 * applies (contiguous 16-byte aligned rows of X, P % 4 == 0); for cross-checks. */
#define MI_LINEAR_VALU 2

/* The rows of the next minibatch drawn by the kernel that reads them (instead of a separate
 * mi_minibatch_rows launch): counter, n, batch, batches_per_epoch, shuffle and seed have
 * mi_minibatch_rows's meaning; the kernel reads the batch number counter[0], draws its rows, writes
 * them to `out` (when non-NULL, for later readers of the batch) and advances counter[0] once all
 * of its blocks have read it (counter[1]: completion count, zero between launches).
 * DataLoader(TensorDataset(X, y), batch_size, shuffle=True) of examples/minibatch.md:78. */
typedef struct mi_rows {
  uint64_t* counter;      /* NULL: no rows drawn here */
  int64_t n;
  int64_t batch;
  int64_t batches;
  uint64_t seed;
  int32_t shuffle;
  int32_t pad0;
  int32_t* out;
} mi_rows;

typedef struct mi_linear {
  int64_t K;
  int64_t N;
  int64_t P;
  int32_t family;
  int32_t options;        /* MI_GROUP_FLAGS_ZEROED | MI_LINEAR_VALU */
  const float* x;         /* X[i, j] at x[i * x_stride_i + j * x_stride_j] */
  int64_t x_stride_i;
  int64_t x_stride_j;
  const float* theta;     /* theta[k, j] at theta[k * theta_stride_k + j * theta_stride_j] */
  int64_t theta_stride_k;
  int64_t theta_stride_j;
  const float* value;     /* value[i * value_stride_i] */
  int64_t value_stride_i;
  const uint8_t* mask;    /* NULL or mask[i * mask_stride_i] */
  int64_t mask_stride_i;
  const float* scale;     /* Normal sigma per particle, or NULL */
  int64_t scale_stride_k;
  float scale_constant;
  float grad_scale;       /* g0 */
  double site_scale;      /* minibatch scale (core.py:267-271) */
  int32_t compute_grads;  /* write dtheta (and dsigma when `scale` is non-NULL) */
  int32_t pad0;
  const int32_t* row_index; /* NULL, or row i of the site reads row row_index[i] of x, value and
                               mask (a device-resident minibatch, mi_minibatch_rows) */
  mi_rows rows;           /* rows.counter non-NULL (row_index NULL): the site draws its batch's
                             rows itself; only the matrix-core kernel with one row stage per
                             block does (else MI_EUNSUPPORTED: launch mi_minibatch_rows first) */
  mi_prior prior;         /* prior.present: a site over theta itself ([K, P], every element; the
                             regression's `theta ~ Normal(0, 1)`, examples/minibatch.md:45-50)
                             evaluated by this launch: its log density joins the site's total,
                             d log p / d theta joins dslots (mi_linear_prior_supported) */
  mi_draw draw;           /* draw.operand != 0: theta is the guide's Normal draw, made by this launch
                             instead of a mi_normal_rsample launch before it (FactorizedDistribution
                             .rsample, nn.py:133-145): theta[k, j] = loc[j] + eps * scale[j] with the
                             eps of mi_normal_rsample (same seed, step, stream, particle_offset + k,
                             element_offset + j; bit-identical values), scale = expf(scale_exp[j])
                             when scale_exp is non-NULL (then also written to scale, as
                             mi_normal_rsample_exp). `theta` is not read; every element of it is
                             written by the launch. dloc / dscale unused. Matrix-core kernel only,
                             P % 4 == 0 (else MI_EUNSUPPORTED: launch mi_normal_rsample first). */
  unsigned long long* stamps; /* as mi_group.stamps: the site kernel's span (timing only) */
  const float* count;     /* MI_BINOMIAL n_i / MI_NEGATIVE_BINOMIAL r_i at count[i * count_stride_i],
                             read through row_index / rows exactly as value is; NULL: every row has
                             count_constant. Data: no gradient, never per particle. Appended to the
                             struct (mi_linear_struct_size grew; a zeroed tail is a valid Normal /
                             Bernoulli site) */
  int64_t count_stride_i;
  float count_constant;
  int32_t pad1;
} mi_linear;

/* *supported = 1 when mi_linear_forward evaluates `site`'s folded prior (the matrix-core kernel). */
int mi_linear_prior_supported(const mi_linear* site, int* supported);

int mi_linear_workspace_bytes(const mi_linear* site, size_t* bytes);
int mi_linear_forward(const mi_linear* site, void* workspace, size_t workspace_bytes, float* total,
                      float* dslots, uint32_t* flags, void* stream);
int mi_linear_struct_size(size_t* bytes);
/* mi_linear_forward with the finalize handed to the caller through *reduce (see mi_reduce); the
 * events as for mi_group_forward_deferred. */
int mi_linear_forward_deferred(const mi_linear* site, void* workspace, size_t workspace_bytes,
                               float* total, float* dslots, uint32_t* flags, void* start_event,
                               void* stop_event, void* stream, mi_reduce* reduce);

/* ---- softmax regression sites (Categorical(logits = X @ Theta)) --------------------------------- */

/* A Categorical site whose logits are the model's own product X @ Theta of an observed design
 * matrix X [N, P] and a per-particle coefficient matrix Theta [K, P, C] (multinomial logistic
 * regression). The product is evaluated inside the site kernel (v_mfma_f32_32x32x2_f32), so the
 * [K, N, C] logits and their gradient never exist in memory. With eta_c = sum_p X[i, p]
 * Theta[k, p, c], m = max_c eta_c and lse = m + log sum_c exp(eta_c - m):
 *   total[k]        = site_scale * sum_i mask_i * (eta_{y_i} - lse)
 *   dtheta[k, p, c] = g0 * site_scale * sum_i mask_i * ([c == y_i] - exp(eta_c - lse)) * X[i, p]
 * (dtheta contiguous [K, P, C], every entry written; not written when NULL). flags[0] (zeroed by
 * the call unless options has MI_GROUP_FLAGS_ZEROED): MI_FLAG_SUPPORT for an observed row whose
 * label is outside [0, C) or (float labels) non-integer or NaN, MI_FLAG_PARAM for a non-finite eta
 * on an observed row; a masked-out row adds nothing and sets no flag, whatever its label holds.
 * MI_EINVAL: a NULL site, x, theta, value, total or flags; K, N, P or C < 1; P > MI_LINEAR_MAX_P;
 * C > MI_SOFTMAX_LINEAR_MAX_C; an unknown value_kind. MI_EWORKSPACE: a workspace smaller than
 * mi_softmax_linear_workspace_bytes asks for. All checked before any device work. */
#define MI_SOFTMAX_LINEAR_MAX_C 32
#define MI_SOFTMAX_LABEL_INT64 0
#define MI_SOFTMAX_LABEL_FLOAT32 1

typedef struct mi_softmax_linear {
  int64_t K;
  int64_t N;
  int64_t P;
  int64_t C;
  const float* x;         /* X[i, j] at x[i * x_stride_i + j * x_stride_j] */
  int64_t x_stride_i;
  int64_t x_stride_j;
  const float* theta;     /* Theta[k, j, c] at theta[k * stride_k + j * stride_j + c * stride_c] */
  int64_t theta_stride_k;
  int64_t theta_stride_j;
  int64_t theta_stride_c;
  const void* value;      /* labels: int64 or float32 (value_kind) at value[i * value_stride_i] */
  int64_t value_stride_i;
  int32_t value_kind;     /* MI_SOFTMAX_LABEL_* */
  int32_t options;        /* MI_GROUP_FLAGS_ZEROED */
  const uint8_t* mask;    /* NULL or mask[i * mask_stride_i] */
  int64_t mask_stride_i;
  const int32_t* row_index; /* NULL, or row i of the site reads row row_index[i] of x, value and
                               mask (as mi_linear.row_index) */
  double site_scale;      /* minibatch scale (core.py:267-271) */
  float grad_scale;       /* g0 */
  int32_t pad0;
} mi_softmax_linear;

int mi_softmax_linear_struct_size(size_t* bytes);
int mi_softmax_linear_workspace_bytes(const mi_softmax_linear* site, size_t* bytes);
int mi_softmax_linear_forward(const mi_softmax_linear* site, void* workspace,
                              size_t workspace_bytes, float* total /* [K] */,
                              float* dtheta /* [K, P, C] contiguous or NULL */, uint32_t* flags,
                              void* stream);

/* ---- group-indexed sites (a parameter indexed by a group label: alpha[group]) -------------------- */

/* A Normal, Bernoulli-logits or Poisson site over N rows of shared data whose parameter is the
 * model's own gather table[index] of a per-particle table [K, G] (a random intercept per group).
 * The gather is evaluated inside the site kernel, so neither the [K, N] parameter nor its [K, N]
 * gradient exists in memory, and the gradient reaches the table without atomics. The site has two
 * parameter roles (Normal: loc, scale; Bernoulli: logits, -; Poisson: rate, -), each one of
 *   MI_GATHER_GATHER    p[k, g_i] = data[k * stride_k + g_i * stride_g], g_i the row's group
 *   MI_GATHER_PARTICLE  data[k * stride_k]
 *   MI_GATHER_DATA      data[i * stride_g]
 *   MI_GATHER_CONSTANT  constant
 * and at least one a GATHER (both may be: they share the index, not the table). A GATHER role is
 * the link of an affine predictor: eta = shift_k + mult_k * p[k, g_i] (shift and mult each absent,
 * one float per particle or a constant), role = eta (MI_GATHER_LINK_IDENTITY) or exp(eta)
 * (MI_GATHER_LINK_EXP). A Poisson site's rate is a GATHER role with the exp link (the log link of
 * the regression: log p = y eta - exp(eta) - lgamma(y + 1)); anything else is MI_EUNSUPPORTED.
 *
 * The index arrives sorted: order[j] is a permutation of the rows, stable-sorted by group, and
 * sorted_group[j] = index[order[j]] (both int32 [N]); value, mask and DATA roles are read at row
 * order[j]. sorted_group must be non-decreasing over all its entries (the launch finds a group's
 * rows by binary search): with an unsorted array no address leaves the buffers, but the sums are
 * undefined. An entry of sorted_group outside [0, G) (or of order outside [0, N)) contributes
 * nothing, is never used as an address and sets MI_FLAG_INTERNAL.
 *   total[k]     = site_scale * sum_i mask_i * log p_i
 *   dtable[k, g] = g0 * site_scale * mult_k * sum_{i: g_i = g} mask_i * d log p_i / d eta
 *                  (grads->role[r] of a GATHER role: contiguous [K, G], every entry written, 0 for
 *                  a group without rows)
 *   grads->role[r] of a PARTICLE role, grads->shift[r], grads->mult[r]: [K], the sums over rows of
 *                  g0 * site_scale * mask_i * d log p_i / d (role | shift | mult)
 * grads, or any pointer in it, may be NULL (not written; those of DATA and CONSTANT roles and of
 * shifts and mults that are not per particle are ignored). flags[0] (zeroed by the call unless
 * options has MI_GROUP_FLAGS_ZEROED): MI_FLAG_SUPPORT for an observed value outside the family's
 * support, MI_FLAG_PARAM for a non-finite eta, a NaN loc or logits or a scale that is not positive
 * on an observed row; a masked-out row adds nothing and sets no flag.
 *
 * A wave's lane takes one particle and walks MI_GATHER_ROWS consecutive sorted rows (a chunk): the
 * rows of a group are consecutive, so its sum stays in a register and is stored once. A group that
 * continues in the neighbouring chunk leaves its part in the workspace ([chunks, K] per role and
 * chunk end); a finishing launch of the same call adds those in chunk order, writes the zeros of
 * the empty groups and sums the chunks' values. No floating-point atomics: two calls on the same
 * inputs give the same bits.
 * MI_EINVAL: a NULL site, order, sorted_group, value, total or flags; K, N or G < 1; an unknown
 * family, kind, link, shift_kind, mult_kind or value_kind; no GATHER role; a GATHER, PARTICLE or
 * DATA role without data; a per-particle shift or mult without its pointer. MI_EWORKSPACE: a
 * workspace smaller than mi_gather_site_workspace_bytes asks for. All checked before any device
 * work. */
#define MI_GATHER_CONSTANT 0
#define MI_GATHER_GATHER 1
#define MI_GATHER_PARTICLE 2
#define MI_GATHER_DATA 3
#define MI_GATHER_LINK_IDENTITY 0
#define MI_GATHER_LINK_EXP 1
#define MI_GATHER_TERM_NONE 0      /* shift = 0, mult = 1 */
#define MI_GATHER_TERM_PARTICLE 1
#define MI_GATHER_TERM_CONSTANT 2
#define MI_GATHER_VALUE_FLOAT32 0
#define MI_GATHER_VALUE_INT64 1
#define MI_GATHER_ROWS 256         /* sorted rows of a chunk */

typedef struct mi_gather_role {
  int32_t kind;           /* MI_GATHER_CONSTANT | GATHER | PARTICLE | DATA */
  int32_t link;           /* MI_GATHER_LINK_* (GATHER roles) */
  const float* data;
  int64_t stride_k;       /* GATHER, PARTICLE: between particles */
  int64_t stride_g;       /* GATHER: between groups; DATA: between rows */
  float constant;
  int32_t shift_kind;     /* MI_GATHER_TERM_* (GATHER roles) */
  int32_t mult_kind;
  float shift_constant;
  float mult_constant;
  int32_t pad0;
  const float* shift;     /* shift[k * shift_stride_k] */
  int64_t shift_stride_k;
  const float* mult;
  int64_t mult_stride_k;
} mi_gather_role;

typedef struct mi_gather_site {
  int64_t K;
  int64_t N;
  int64_t G;
  int32_t family;         /* MI_NORMAL, MI_BERNOULLI_LOGITS or MI_POISSON */
  int32_t options;        /* MI_GROUP_FLAGS_ZEROED */
  mi_gather_role role[2];
  const int32_t* order;         /* [N] */
  const int32_t* sorted_group;  /* [N] */
  const void* value;      /* float32 or int64 (value_kind) at value[i * value_stride_i] */
  int64_t value_stride_i;
  int32_t value_kind;     /* MI_GATHER_VALUE_* */
  int32_t pad0;
  const uint8_t* mask;    /* NULL or mask[i * mask_stride_i] */
  int64_t mask_stride_i;
  double site_scale;      /* minibatch scale (core.py:267-271) */
  float grad_scale;       /* g0 */
  int32_t pad1;
} mi_gather_site;

typedef struct mi_gather_grads {
  float* role[2];
  float* shift[2];
  float* mult[2];
} mi_gather_grads;

int mi_gather_site_struct_size(size_t* bytes);
int mi_gather_site_workspace_bytes(const mi_gather_site* site, size_t* bytes);
int mi_gather_site_forward(const mi_gather_site* site, void* workspace, size_t workspace_bytes,
                           float* total /* [K] */, const mi_gather_grads* grads /* or NULL */,
                           uint32_t* flags, void* stream);

/* A group-indexed site whose first role also has fixed effects: the varying intercept plus linear
 * predictor of a multilevel regression,
 *   eta0[k, i] = shift_k + mult_k * p[k, g_i] + sum_{j < P} X[i, j] * theta[k, j],
 * role 0 = eta0 (MI_GATHER_LINK_IDENTITY) or exp(eta0) (MI_GATHER_LINK_EXP). `site` is a
 * mi_gather_site whose role[0] is a GATHER role; role[1] is any kind mi_gather_site takes. X is
 * read at x[i * x_stride_i + j * x_stride_j] (rows at i = order[j'], like value, mask and DATA
 * roles), theta at theta[k * theta_stride_k + j * theta_stride_j]. Neither the [K, N] predictor
 * nor a gradient of its shape exists in memory.
 *   total, grads: as documented for mi_gather_site, with role 0's eta extended by the linear term
 *   dtheta[k, j] = g0 * site_scale * sum_i mask_i * (d log p_i / d eta0) * X[i, j]
 *                  (contiguous [K, P], every entry written; NULL: not wanted), d log p_i / d eta0
 *                  the per-row quantity summed into role 0's dtable, a link's chain factor included
 * flags as for mi_gather_site; a non-finite eta0 is a per-row condition here (a non-finite entry
 * of theta, or of X on an observed row, sets MI_FLAG_PARAM). A masked-out row adds nothing and
 * sets no flag.
 *
 * The layout is mi_gather_site's: a lane owns one particle and walks MI_GATHER_ROWS consecutive
 * sorted rows, a group's sum stays in the lane, neighbours' parts meet in the workspace in chunk
 * order. eta0 changes with every row, so the density's terms are derived per row. The lane holds
 * theta[k, 0..P) and the P sums of dtheta in registers (a float over a batch of 8 rows folded into
 * a float over the chunk: at most 8 + 32 roundings of a sum), every lane of a particle tile reads
 * a row of X at one address, and the chunk's P sums leave the lane once, into a workspace slab
 * [P][chunks][K] that a finishing launch adds in chunk order in fp64. No floating-point atomics:
 * two calls on the same inputs give the same bits. The workspace is mi_gather_site's plus
 * K * P * ceil(N / MI_GATHER_ROWS) floats.
 * MI_EINVAL: those of mi_gather_site, and a role[0] that is not a GATHER role, P < 1, a NULL x or
 * theta. MI_EUNSUPPORTED: those of mi_gather_site, and P > MI_GATHER_LINEAR_MAX_P (from
 * mi_gather_linear_workspace_bytes too). MI_EWORKSPACE: a workspace smaller than
 * mi_gather_linear_workspace_bytes asks for. All checked before any device work. */
#define MI_GATHER_LINEAR_MAX_P 32
typedef struct mi_gather_linear {
  mi_gather_site site;    /* role[0] must be a GATHER role */
  int64_t P;
  const float* x;         /* X[i, j] at x[i * x_stride_i + j * x_stride_j] */
  int64_t x_stride_i;
  int64_t x_stride_j;
  const float* theta;     /* theta[k, j] at theta[k * theta_stride_k + j * theta_stride_j] */
  int64_t theta_stride_k;
  int64_t theta_stride_j;
} mi_gather_linear;

int mi_gather_linear_struct_size(size_t* bytes);
int mi_gather_linear_workspace_bytes(const mi_gather_linear* site, size_t* bytes);
int mi_gather_linear_forward(const mi_gather_linear* site, void* workspace, size_t workspace_bytes,
                             float* total /* [K] */, const mi_gather_grads* grads /* or NULL */,
                             float* dtheta /* [K, P] contiguous or NULL */, uint32_t* flags,
                             void* stream);

/* A group-indexed site with varying slopes: the predictor of role 0 is
 *   eta0[k, i] = shift_k + mult_k * p[k, g_i] + sum_{s < S} beta_s[k, g_i] * z_s[i]
 *              + sum_{j < P} X[i, j] * theta[k, j],
 * 1 <= S <= MI_GATHER_MAX_SLOPES slope terms, each a per-particle table beta_s [K, G] gathered by
 * the site's index (slope[s].table[k * stride_k + g * stride_g]) times an observed float32 column
 * z_s [N] (slope[s].z[i * z_stride_i], rows at i = order[j'] like value, mask and X), and
 * 0 <= P <= MI_GATHER_LINEAR_MAX_P fixed effects (`linear`, a mi_gather_linear whose P may be 0: x
 * and theta are then not read and may be NULL). Families, links, role 1, mask, values, site_scale
 * and grad_scale are mi_gather_linear's. eta0 is evaluated in float32 in a fixed order:
 * fmaf(mult, p, shift), one fmaf(beta_s, z_s, eta) per slope s = 0..S-1, one fmaf(X[i, j],
 * theta[j], eta) per column j = 0..P-1.
 *   total, grads, dtheta: as documented for mi_gather_linear, with the slope terms inside eta0
 *                  (dtheta is not touched when P = 0)
 *   dslope[s][k, g] = g0 * site_scale * sum_{i in g} mask_i * (d log p_i / d eta0) * z_s[i]
 *                  (contiguous [K, G], every entry written, a group without rows exactly 0; a NULL
 *                  entry, or a NULL array, is not wanted), d log p_i / d eta0 the per-row quantity
 *                  summed into role 0's dtable and into dtheta
 * flags as for mi_gather_linear: a non-finite beta_s entry of a group with an observed row, or a
 * non-finite z_s on an observed row, sets MI_FLAG_PARAM through the non-finite eta0. A masked-out
 * row reads no z, adds nothing and sets no flag.
 *
 * The layout is mi_gather_linear's. A lane loads beta_s[k, g] when the group changes and keeps one
 * more sum per slope (a float over a batch of 8 rows folded into a double), stored to dslope when
 * the group ends; the part of a group that continues in a neighbouring chunk goes to a workspace
 * slab [S][2 ends][chunks][K] that a finishing launch adds in chunk order in fp64 (it also writes
 * the zeros of the empty groups). No floating-point atomics: two calls on the same inputs give the
 * same bits. The workspace is mi_gather_linear's (with P as given) plus that slab.
 * MI_EINVAL: those of mi_gather_site, and a role[0] that is not a GATHER role, S < 1, a NULL table
 * or z among the first S slopes, P < 0, P >= 1 with a NULL x or theta. MI_EUNSUPPORTED: those of
 * mi_gather_site, S > MI_GATHER_MAX_SLOPES and P > MI_GATHER_LINEAR_MAX_P (from
 * mi_gather_slopes_workspace_bytes too). MI_EWORKSPACE: a workspace smaller than
 * mi_gather_slopes_workspace_bytes asks for. All checked before any device work. */
#define MI_GATHER_MAX_SLOPES 4
typedef struct mi_gather_slope {
  const float* table;     /* beta_s[k, g] at table[k * stride_k + g * stride_g] */
  int64_t stride_k;
  int64_t stride_g;
  const float* z;         /* z_s[i] at z[i * z_stride_i] */
  int64_t z_stride_i;
} mi_gather_slope;

typedef struct mi_gather_slopes {
  mi_gather_linear linear;   /* site.role[0] must be a GATHER role; P may be 0 */
  int64_t S;
  mi_gather_slope slope[MI_GATHER_MAX_SLOPES];
} mi_gather_slopes;

int mi_gather_slopes_struct_size(size_t* bytes);
int mi_gather_slopes_workspace_bytes(const mi_gather_slopes* site, size_t* bytes);
int mi_gather_slopes_forward(const mi_gather_slopes* site, void* workspace, size_t workspace_bytes,
                             float* total /* [K] */, const mi_gather_grads* grads /* or NULL */,
                             float* dtheta /* [K, P] contiguous or NULL */,
                             float* const dslope[MI_GATHER_MAX_SLOPES] /* or NULL */,
                             uint32_t* flags, void* stream);

/* ---- device-resident minibatches (replaces examples/minibatch.md:78-88, the host DataLoader) ---- */

/* Row indices of the next minibatch of an n-row dataset: with c = counter[0] (then counter[0] =
 * c + 1, in the same launch; counter[1] is the launch's completion count and must be zero
 * initially -- every launch leaves it at zero), epoch e = c / batches_per_epoch and batch
 * b = c % batches_per_epoch,
 *   rows[j] = perm_e(b * batch + j)  (shuffle)   or   b * batch + j,   j < count,
 * where perm_e is a keyed Feistel permutation of [0, n) (seed, e): a fresh random order every
 * epoch, like DataLoader(..., shuffle=True) (dataloader.py RandomSampler), computed on the device.
 * count is batch, or the shorter last batch of an epoch (batch b * batch + count <= n; positions
 * past the data are not permuted). batches_per_epoch is ceil or floor of n / batch. n < 2^31. */
int mi_minibatch_rows(uint64_t* counter, int64_t n, int64_t batch, int64_t batches_per_epoch,
                      int32_t shuffle, uint64_t seed, int32_t* rows, int64_t count, void* stream);

/* out[j] = base[rows[j]]: count rows of row_bytes bytes (multiples of 4) -- a minibatch
 * materialised for uses other than the site kernels that read rows through the index. */
int mi_gather_rows(const void* base, int64_t base_stride_bytes, int64_t row_bytes,
                   const int32_t* rows, int64_t count, void* out, int64_t out_stride_bytes,
                   void* stream);

/* ---- optimizer step (replaces torch.optim.Adam.step of the training loop, README.md:66-69) ----- */

/* One Adam step for up to MI_ADAM_MAX_TENSORS fp32 parameters in one launch, arithmetic of torch's
 * fused Adam (fused_adam_utils.cuh adam_math: ADAM_MODE::ORIGINAL, no AMSGrad):
 *   s = *step + 1;  g = (maximize ? -grad : grad) + weight_decay * param
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   param -= lr / (1 - beta1^s) * m / (sqrt(v) / sqrt(1 - beta2^s) + eps);  *step = s
 * per tensor (its own step word, fp32 as torch keeps it). `counters`: MI_ADAM_COUNTER_WORDS uint32
 * words, zero before first use, owned by one caller's launches on one stream: the completion
 * counters (every launch leaves them zero), then a cache of the next step's bias corrections per
 * tensor slot (ABI 16; a slot that does not match the step and betas is recomputed). */
#define MI_ADAM_MAX_TENSORS 8
#define MI_ADAM_COUNTER_WORDS (MI_ADAM_MAX_TENSORS * 33 + MI_ADAM_MAX_TENSORS * 16)
typedef struct mi_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  int64_t numel;          /* contiguous */
} mi_adam_tensor;
typedef struct mi_adam {
  int32_t num;
  int32_t maximize;
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  mi_adam_tensor tensors[MI_ADAM_MAX_TENSORS];
} mi_adam;
int mi_adam_step(const mi_adam* adam, uint32_t* counters, void* stream);

/* ---- one-shot peer-write all-reduce (replaces the sharded step's small-bucket
 * dist.all_reduce / ncclAllReduce, distributed.GradientBucket) -------------------------------------
 * Each rank allocates one region (mi_peer_region_bytes for the largest bucket, mi_peer_alloc:
 * fine-grained device memory, zeroed, and its IPC handle, MI_PEER_HANDLE_BYTES), exchanges the
 * handles over its process group and maps the peers' regions (mi_peer_open). mi_peer_allreduce
 * then sums a float bucket over the ranks in ONE kernel on the caller's stream (capturable): the
 * bucket is written into a slot of every peer's region with system-scope stores, a flag carrying
 * the call number follows, the caller waits for every peer's flag in its own region and adds the
 * slots in rank order (two ranks: the same sum as any SUM all-reduce). A peer that never arrives
 * ends the wait after about a second: the call sets bit 0 of *error (device-visible memory, e.g.
 * pinned host memory the host can poll; never cleared by the library), fills `out` with NaN and
 * does not advance the call counter. A call that finds *error set at entry does the same without
 * writing into any peer's region (sticky failure: the communicator is unusable afterwards). Every
 * rank must call it the same number of times, with buckets of the same length. */
#define MI_PEER_MAX_RANKS 8
#define MI_PEER_MAX_FLOATS 4096
#define MI_PEER_HANDLE_BYTES 64
typedef struct mi_peer {
  int32_t rank;
  int32_t world;
  int64_t max_floats;                    /* the regions' slot length */
  void* regions[MI_PEER_MAX_RANKS];      /* [rank]: this rank's region; others: the mapped peers' */
} mi_peer;
int mi_peer_region_bytes(int64_t max_floats, size_t* bytes);
int mi_peer_alloc(size_t bytes, void** region, void* handle);
int mi_peer_open(const void* handle, void** region);
int mi_peer_close(void* region);
int mi_peer_free(void* region);
int mi_peer_allreduce(const mi_peer* peer, const float* in, float* out, int64_t n,
                      uint32_t* error, void* stream);
/* Diagnostics (synchronous): the number of calls this rank's region has completed. */
int mi_peer_call_count(const mi_peer* peer, uint64_t* count);

/* ---- ELBO tail (replaces nn.py:224-228 + FactorizedDistribution.entropy, nn.py:121-131) -------- */

#define MI_MAX_TERMS 8
#define MI_MAX_FACTORS 8
#define MI_MAX_BUFFERS 16

/* One mean-field guide factor whose entropy enters the ELBO, viewed as n elements:
 *   MI_NORMAL: param[0] = loc (read only with an absorbed draw), param[1] = scale
 *   MI_BETA:   param[0] = concentration1, param[1] = concentration0
 *   MI_GAMMA:  param[0] = concentration, param[1] = rate (gamma.py:101-107; draw_kind NONE only)
 * Parameters are fp32 with element stride `stride` (0 only when n == 1). mi_elbo_backward writes
 *   grad[j][i * grad_stride[j]] = d loss / d param_j(i)                  (transform[j] NONE)
 *                               = d loss / d u_j(i) = (d loss / d param_j) * param_j
 *                                                       (transform[j] EXP: param_j = exp(u_j))
 * for every non-NULL grad[j]. The transforms restate ParameterizedDistribution's
 * transform_to(constraint) (nn.py:86-96): EXP is transform_to(positive) = exp.
 *
 * Absorbed guide draw (draw_kind != MI_DRAW_NONE). The factor's K draws z (Normal: z = loc +
 * eps * scale, normal.py:83-86; Beta: implicit reparameterisation, dirichlet.py:17-20) feed only
 * site kernels of this ELBO, so d loss / d param also carries the draws' backward (what
 * mi_normal_rsample_backward / mi_beta_rsample_backward and autograd's accumulation would add):
 *   MI_DRAW_SOURCES:  dz[k, i] = sum_s source[s].ptr[k * stride_k + i * stride_i]  (pre-scaled by
 *                     g0, like every speculative site gradient); Normal: eps from the generator
 *                     (seed, step, step_device, stream_id, particle_offset) or `eps` [K, n];
 *                     Beta: `draws` holds x [K, n] row-major.
 *   MI_DRAW_PARTIALS: Normal draws fused into a site group (mi_draw): partial[0] / partial[1] hold
 *                     partial_rows rows [rows, n] of sum_k g0 dT/dz and sum_k g0 dT/dz * eps. */
#define MI_TRANSFORM_NONE 0
#define MI_TRANSFORM_EXP 1
#define MI_DRAW_NONE 0
#define MI_DRAW_SOURCES 1
#define MI_DRAW_PARTIALS 2
#define MI_MAX_SOURCES 4

typedef struct mi_source {
  const float* ptr;
  int64_t stride_k;
  int64_t stride_i;
} mi_source;

typedef struct mi_factor {
  int32_t family;
  int32_t draw_kind;            /* MI_DRAW_* */
  int64_t n;
  const float* param[2];
  int64_t stride[2];
  float* grad[2];
  int64_t grad_stride[2];
  int32_t transform[2];         /* MI_TRANSFORM_* per parameter */
  int32_t num_sources;
  uint32_t stream_id;
  mi_source source[MI_MAX_SOURCES];
  const float* draws;           /* Beta draws x [K, n] */
  const float* eps;             /* Normal: injected noise [K, n], or NULL to regenerate */
  uint64_t seed;
  uint64_t step;
  const uint64_t* step_device;  /* may be NULL; added to step */
  int64_t particle_offset;
  const float* partial[2];      /* MI_DRAW_PARTIALS */
  int64_t partial_rows;
  const double* dgrad;          /* Beta, MI_DRAW_SOURCES: mi_beta_dgrad output [K, n, 2], or NULL
                                   to evaluate the implicit gradients in mi_elbo_forward */
  double* saved;                /* Beta, MI_DRAW_SOURCES: [n, 4] fp64 sums mi_elbo_forward writes
                                   and mi_elbo_backward of the same evaluation reads (required).
                                   Owned by the caller per evaluation, so evaluations sharing a
                                   workspace may interleave (loss1 + loss2, then backward). */
  int64_t element_offset;       /* Normal, regenerated eps: the draw's mi_draw.element_offset */
  double weight;                /* this factor's entropy enters as entropy_scale * weight * H_f:
                                   1 for a factor every rank holds whole or owns a slice of, 1/W
                                   for one replicated on W data-sharded ranks; > 0 (a zeroed
                                   descriptor is rejected) */
} mi_factor;

/* loss = g0 * sum_t sum_k terms[t][k] - entropy_scale * sum_f weight_f * sum_i H_f(i)
 * terms: per-particle log joints [K] (site-group totals, categorical totals, torch-evaluated sites);
 * g0 = -1/K_total (fp32); entropy_scale = 1/world when particles are sharded over ranks.
 * buffers: the speculative gradients of the site groups (computed for upstream g0), rescaled by
 * mi_elbo_backward when the loss's upstream gradient is not exactly 1. */
typedef struct mi_elbo {
  int64_t K;
  int32_t num_terms;
  int32_t num_factors;
  int32_t num_buffers;
  int32_t num_reduce;
  float g0;
  int32_t options;       /* MI_ELBO_* bits */
  double entropy_scale;
  const float* terms[MI_MAX_TERMS];
  mi_factor factors[MI_MAX_FACTORS];
  float* buffers[MI_MAX_BUFFERS];
  int64_t buffer_len[MI_MAX_BUFFERS];
  /* deferred site finalize reductions (same K): mi_elbo_forward writes their outputs and adds
   * g0 * sum_k total[k] of each to the loss (their totals are not listed in `terms`). Forward-
   * absorbed Beta factors (MI_DRAW_SOURCES) must then have `dgrad`: their sums over the particles
   * (which read slot gradients the reductions write) move to mi_elbo_backward. */
  mi_reduce reduce[MI_MAX_REDUCE];
  /* step_counter != NULL: after everything else, the launch's last block sets
   * *step_snapshot = *step_counter and *step_counter += 1 (the generator step of this ELBO
   * evaluation's draws -- read from step_counter in the forward, from step_snapshot afterwards). */
  uint64_t* step_counter;
  uint64_t* step_snapshot;
  /* flags_mirror != NULL: the last block copies flags[0 .. nflags) there (e.g. host-mapped memory:
   * the validation words of this evaluation without a separate device-to-host copy). */
  const uint32_t* flags;
  uint32_t* flags_mirror;
  int64_t nflags;
} mi_elbo;


/* mi_elbo.options: the forward's last block also writes the final gradients (`grad` of every
 * factor) for an upstream gradient of exactly 1 -- loss.backward() of the training loop,
 * README.md:66-69 -- when mi_elbo_final_grads reports the forward complete; the caller then need not
 * launch mi_elbo_backward for that upstream (any other upstream: launch it, it rewrites them). */
#define MI_ELBO_FINAL_GRADS 1

/* *complete = 1 when mi_elbo_forward with MI_ELBO_FINAL_GRADS leaves nothing for mi_elbo_backward
 * at an upstream of 1: every factor is a one-element forward-absorbed Beta factor whose sums the
 * forward finishes (the README model's theta, with deferred site reductions). */
int mi_elbo_final_grads(const mi_elbo* elbo, int* complete);

/* sizeof(mi_factor), sizeof(mi_elbo) as compiled. */
int mi_elbo_struct_sizes(size_t* factor, size_t* elbo);

/* Workspace of mi_elbo_forward and mi_elbo_backward. Its first MI_ELBO_COUNTER_BYTES hold
 * completion counters that must be zero before first use (mi_elbo_workspace_init) and that every
 * launch leaves at zero, so one workspace serves every step (and captured HIP graphs) on one
 * stream. */
#define MI_ELBO_COUNTER_BYTES 16640
int mi_elbo_workspace_bytes(const mi_elbo* elbo, size_t* bytes);
int mi_elbo_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* Writes the scalar loss (fp32, reduced in fp64 in a fixed order). MI_EUNSUPPORTED when num_reduce
 * > 0 and a forward-absorbed Beta factor has no dgrad (see mi_elbo.reduce). A launch too large to
 * reduce its jobs itself runs them as launches of their own first; of a job with particle-summed
 * values (mi_reduce.ksum) it runs the slots that way and adds the doubles in its lead blocks. */
int mi_elbo_forward(const mi_elbo* elbo, void* workspace, size_t workspace_bytes, float* loss,
                    void* stream);

/* The optimizer step of the factors an ELBO forward finishes (ABI 14). With MI_ELBO_FINAL_GRADS
 * the forward's last block writes the gradients of one-element Beta tails and of the Normal tail
 * (nt) for an upstream of 1; mi_elbo_forward_adam also runs Adam there, on the unconstrained tensor
 * behind factor `factor`'s parameter `param` (mi_factor.grad[param] is its gradient), with
 * mi_adam_step's arithmetic (torch's fused Adam): the update, the moments and the step count, by
 * the thread that writes the gradient -- no optimizer launch for the step. `adam` is a DEVICE
 * pointer (the descriptor is read by the kernel; it may be reused across launches); NULL: as
 * mi_elbo_forward. mi_elbo_adam_supported checks a HOST copy against the launch: every slot's
 * factor finished by the last block, numel = the factor's n, the gradient written, no
 * (factor, param) twice; a fused-draw factor's slots are declined (mi_adam_step streams them at
 * full occupancy). Replaces optimizer.step() (README.md:66-69) for those parameters. */
#define MI_ELBO_ADAM_SLOTS 4
typedef struct mi_elbo_adam_slot {
  int32_t factor;
  int32_t param;
  float* value;           /* the optimised tensor (contiguous, numel = the factor's n) */
  float* exp_avg;
  float* exp_avg_sq;
  float* step;            /* one float */
  int64_t numel;
} mi_elbo_adam_slot;
typedef struct mi_elbo_adam {
  int32_t num;
  int32_t maximize;
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  mi_elbo_adam_slot slots[MI_ELBO_ADAM_SLOTS];
} mi_elbo_adam;
int mi_elbo_adam_supported(const mi_elbo* elbo, const mi_elbo_adam* adam, int* supported);
int mi_elbo_forward_adam(const mi_elbo* elbo, void* workspace, size_t workspace_bytes,
                         float* loss, const mi_elbo_adam* adam, void* stream);

/* With u = *upstream (device scalar, d out / d loss): dterm[0] = u * g0 (the gradient of every
 * term element); factors[f].grad[j] = the gradient of -u * entropy_scale * H_f (plus u times the
 * absorbed draw's backward, and the transform's chain rule; see mi_factor); every buffer is
 * multiplied by u unless u == 1. One launch; `workspace` is the mi_elbo_forward workspace. */
int mi_elbo_backward(const mi_elbo* elbo, const float* upstream, float* dterm, void* workspace,
                     size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MININF_AMD_H */
