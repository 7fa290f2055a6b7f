// The 32 x 32 tile toolkit of the guide samplers that run on v_mfma_f32_32x32x2_f32
// (mvn_guide.hip, lowrank_guide.hip): tiles staged in LDS rows of 33 floats, the Philox normals (or
// the injected eps) of a tile, a strided dz tile, and the 16-step MFMA walk over two staged tiles.
// Nothing here knows a family: what a kernel stages, and for whom, stays in the kernel.
#pragma once

#include "common.hpp"

namespace mi {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileThreads = 256;         // a block of the MFMA kernels: four waves, a tile each
constexpr int kTileWaves = kTileThreads / kWave;
constexpr int kTile = 32;
constexpr int kTileStride = kTile + 1;    // LDS row stride: column and row reads both conflict-free
constexpr int kTileFloats = kTile * kTileStride;

// The C/D row of accumulator register r (32x32 MFMA: the column is lane & 31).
MI_DEV int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// A factor's Normal stream, or the injected eps that replaces it (row-major [K, eps_ld]).
struct NormalsKey {
  uint64_t seed, step;
  uint32_t stream_id;
  int64_t poff;
  const float* eps_in;
  int64_t eps_ld;
};

// Where a section of the factor's normals lives in the stream and in the injected eps.
struct NormalsSection {
  int64_t n;        // elements in the section
  int64_t quad0;    // first Philox quad of the section
  int64_t in_off;   // first column of the section in the injected eps
};

// The four normals of particle k, section elements j0 .. j0 + 3 (j0 a multiple of 4), zero
// outside K x n.
MI_DEV void normals_quad(const NormalsKey& key, const NormalsSection& sec, int64_t k, int64_t K,
                         int64_t j0, float e[4]) {
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (k < K && j0 < sec.n) {
    if (key.eps_in != nullptr) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[c] = (j0 + c < sec.n) ? key.eps_in[k * key.eps_ld + sec.in_off + j0 + c] : 0.0f;
    } else {
      guide_normals(key.seed, key.step, key.stream_id, (uint64_t)(sec.quad0 + (j0 >> 2)),
                    (uint64_t)(key.poff + k), v);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) e[c] = (j0 + c < sec.n) ? v[c] : 0.0f;
}

// Stage the normals of particles [kbase, kbase + 32) x section elements [e0, e0 + 32) into
// tile[particle][element]: quad t of the tile's 256 ...
MI_DEV void stage_quad(float* __restrict__ tile, const NormalsKey& key, const NormalsSection& sec,
                       int64_t kbase, int64_t K, int64_t e0, int t) {
  const int q = t & 7, p = t >> 3;
  float e[4];
  normals_quad(key, sec, kbase + p, K, e0 + 4 * q, e);
#pragma unroll
  for (int c = 0; c < 4; ++c) tile[p * kTileStride + 4 * q + c] = e[c];
}

// ... and quads `first`, `first + STEP`, ...: a block stages a tile with <kTileThreads>(threadIdx.x),
// one quad per thread and no loop; a wave with <kWave>(lane).
template <int STEP>
MI_DEV void stage_tile(float* __restrict__ tile, const NormalsKey& key, const NormalsSection& sec,
                       int64_t kbase, int64_t K, int64_t e0, int first) {
  if constexpr (STEP == kTile * 8) {
    stage_quad(tile, key, sec, kbase, K, e0, first);
  } else {
    for (int t = first; t < kTile * 8; t += STEP) stage_quad(tile, key, sec, kbase, K, e0, t);
  }
}

// Step r of 16 of a wave staging dz of particles [kbase, kbase + 32) x elements
// [ibase, ibase + 32) into tile[particle][element] (zero outside K x D). Lanes run along the
// unit-stride axis of dz; the values and the tile do not depend on which. The unrolled loop over r
// must stay in the calling kernel (inside this helper it costs the kernels registers).
MI_DEV void stage_dz_row(float* tile, const float* __restrict__ dz, int64_t dz_sk, int64_t dz_si,
                         int64_t kbase, int64_t K, int64_t ibase, int64_t D, int r, int lane) {
  const int col = lane & 31, half = lane >> 5;
  const bool along_i = dz_si == 1 || dz_sk != 1;
  const int kk = along_i ? 2 * r + half : col;
  const int ii = along_i ? col : 2 * r + half;
  const int64_t k = kbase + kk, i = ibase + ii;
  tile[kk * kTileStride + ii] = (k < K && i < D) ? dz[k * dz_sk + i * dz_si] : 0.0f;
}

// acc[m][n] += sum_k a[m][k] b[n][k] over the 32 k of two staged tiles, k ascending: the forward
// products, A = eps[particle][k] and B = the factor's [element][k] tile.
MI_DEV void mfma_tile_nt(f32x16& acc, const float* a, const float* b, int lane) {
  const int col = lane & 31, half = lane >> 5;
#pragma unroll
  for (int s = 0; s < 16; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[col * kTileStride + 2 * s + half],
                                               b[col * kTileStride + 2 * s + half], acc, 0, 0, 0);
}

// Step s of the walk over k-major tiles, t[k][m] (the backward products, whose loops also carry
// the dloc / dd sums of the A operand): this lane's operand.
MI_DEV float tile_k_major(const float* t, int s, int lane) {
  return t[(2 * s + (lane >> 5)) * kTileStride + (lane & 31)];
}

}  // namespace mi
