// Host-side helpers shared between the library's translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int to_code(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

constexpr int64_t kMaxGrid = 0x7FFFFFFF;   // blocks along x of a grid

// Launch geometry of the particle-reducing sampler backwards (guide.hip, dirichlet.hip): blocks of
// `threads`, `ti` element lanes (min(64, next_pow2(units))) x threads / ti particle lanes, and
// enough particle slices of `rows` particles to fill the chip.
struct BwdGeometry {
  int ti;
  int64_t gx, slices, rows;
};

inline BwdGeometry bwd_geometry(int64_t K, int64_t units, int threads) {
  BwdGeometry g{};
  int ti = 1;
  while (ti < 64 && ti < units) ti <<= 1;
  g.ti = ti;
  const int tk = threads / ti;
  g.gx = ceil_div(units, ti);
  int64_t slices = ceil_div(1024, g.gx);
  slices = std::min<int64_t>(slices, ceil_div(K, (int64_t)tk * 2));
  slices = std::max<int64_t>(1, slices);
  g.rows = ceil_div(K, slices);
  g.slices = ceil_div(K, g.rows);
  return g;
}

// The tail every sliced sampler backward shares. A workspace of `need` bytes was asked for (none:
// any pointer does) ...
inline bool workspace_ok(const void* workspace, size_t bytes, size_t need) {
  return need == 0 || (workspace != nullptr && bytes >= need);
}
// ... and with more than one particle slice the kernel writes per-slice partials at float
// `offset` of the workspace instead of the output itself (a slice-summing launch follows).
inline float* slice_out(float* out, void* workspace, int64_t slices, int64_t offset) {
  return slices > 1 ? static_cast<float*>(workspace) + offset : out;
}

// Fixed-order fp64 reduction of per-(segment, particle) partials part[v][nseg][K] (reduce.hip
// k_finalize): values v < num_sites are multiplied by scale[v] and summed into total[k] (and
// written to site_lp[v*K + k] when non-NULL); the remaining num_slots values are multiplied by
// slot_scale and written to slot_grad[(v - num_sites)*K + k].
// With long segment lists (> 512) and a `scratch` of mi_finalize_scratch_bytes, the reduction
// runs in two launches (segment chunks in parallel, then the chunk sums); otherwise in one.
size_t mi_finalize_scratch_bytes(int64_t nseg, int64_t K, int nv);
// rank1: bit v marks value v as stored in mi_reduce's rank-one layout (one-launch path only).
int mi_launch_finalize(const float* part, int64_t nseg, int64_t K, int num_sites, int num_slots,
                       const double* scale, double slot_scale, float* total, double* site_lp,
                       float* slot_grad, double* scratch, hipStream_t stream, int rank1 = 0,
                       int ksum = 0);
// ksum: bit v marks site value v as particle-summed (mi_reduce.ksum): it has no block in `part`
// (the later values' blocks move up), is skipped, and `total` is not written.

// The slot values of a job whose site values are particle-summed (mi_reduce.ksum != 0), as their
// own launch: what mi_elbo_forward runs for such a job when the launch is too large to reduce its
// jobs itself (its lead blocks then add the job's doubles).
struct mi_reduce;
int mi_reduce_launch_slots(const mi_reduce* r, void* stream);

// The per-K-block dloc / dscale partials of a fused guide draw, part[2][slices][N], summed over the
// slices in a fixed order (reduce.hip k_draw_reduce).
int mi_launch_draw_reduce(const float* part, int64_t slices, int64_t N, float* dloc, float* dscale,
                          hipStream_t stream);

// Timing events around a site kernel (the `start_event` / `stop_event` arguments) are for eager
// launches only. Round 5 first recorded them under capture with hipEventRecordWithFlags(...,
// hipEventRecordExternal) (commit c13b392): on this stack that call returns hipErrorInvalidValue
// inside a capture, which invalidates the whole capture sequence, so the draw launched next
// (mi_normal_rsample_exp) failed with the same code (gpurun_out/dbg1_one.err). Replayed kernels
// are timed by span stamps instead (mi_group.stamps / mi_linear.stamps). An entry point given
// events while `stream` is capturing returns MI_EUNSUPPORTED before it enqueues anything, so the
// capture stays valid.
inline hipError_t mi_stream_capturing(hipStream_t stream, bool* capturing) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(stream, &status);
  *capturing = status != hipStreamCaptureStatusNone;
  return e;
}

inline hipError_t mi_record_event(void* event, hipStream_t stream) {
  return hipEventRecord(static_cast<hipEvent_t>(event), stream);
}
