// What the launch planner (sites.hip) needs from the broadcast site unit (bcast_site.hip): the
// constants its grids and workspace layout are made of, the host tests that choose between the two
// BCAST kernels, and one launch function for each.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mininf_amd.h"

namespace mi {

constexpr int kBcastThreads = 256;
constexpr int kBcastP = 8;          // particles per lane
constexpr int kBcastChunk = 2048;   // elements staged per block
constexpr int kPrep = 5;            // per-particle constants of a k_site_bcast launch (k_bcast_prep)
constexpr int kSmemMaxChunk = 4096; // longest chunk of a k_site_bcast_smem launch (smem_chunk)

// k_site_bcast_smem: particles per lane and chunk length (measured r02: the best of {4, 8} x
// {2048, 4096, 8192}; r06 at 78 VGPR: 8 particles per lane in 1010 workgroups 91.8 us per C2 step
// against 86.2, profiles/r06_ab.json ab14)
constexpr int kSmemP = 4;

// The side job's workgroups, as the plan (make_plan) and the kernel count them.
__host__ __device__ inline int64_t beta_side_blocks(const mi_side& S) {
  return S.out != nullptr ? (2 * S.K * S.N + kBcastThreads - 1) / kBcastThreads : 0;
}

// Whether the group is one site of the BCAST shape at all, and whether it is a Bernoulli site over
// unmasked contiguous data: k_site_bcast_smem instead of k_bcast_prep + k_site_bcast.
bool bcast_eligible(const mi_group* g);
bool bcast_smem(const mi_group* g);

// k_site_bcast_smem: elements per chunk for N elements and gy particle blocks; and whether a launch
// of nseg segments writes its slot value in the rank-one layout (mi_reduce.rank1).
int smem_chunk(int64_t N, int64_t gy);
bool smem_rank1(const mi_group* g, int64_t nseg);

// k_bcast_prep into `prep`, then k_site_bcast on `grid` (chunks, particle blocks). `start_event`
// (or NULL) is recorded between the two: eager timing brackets the site kernel alone. Returns 0 or
// an MI_E* / hipError_t code; launch errors are left for the caller's hipGetLastError.
int bcast_launch(const mi_group& G, float* prep, float* part, int64_t nseg, dim3 grid,
                 uint32_t* flags, void* start_event, hipStream_t stream);

// k_site_bcast_smem for the plan's grid (chunks + side blocks, particle blocks) and chunk length;
// `ksum` (or NULL): where the particle-summed site values go (MI_GROUP_KSUM).
void bcast_launch_smem(const mi_group& G, float* part, int64_t nseg, dim3 grid, int chunk,
                       uint32_t* flags, double* ksum, hipStream_t stream);

}  // namespace mi
