// literal_cell.h -- the literal cell of the traceback kernels: a 16-byte state
// cell unpacked, the literal MAX7 with its argmax, and the pointer cube index.
// Shared by the plane sweep (plane_kernel.hip) and the resident traceback
// kernels (align_step.h), which must pick the same winner at every cell.
#pragma once

#include "tsa_internal.h"

namespace tsa {

__device__ __forceinline__ int32_t wrapv(int32_t v, int32_t sh) { return (v << sh) >> sh; }

// The 7 states of a staged cell, sign-extended.
__device__ __forceinline__ void unpack7(uint4 c, int32_t (&v)[7]) {
  v[0] = (int16_t)(c.x & 0xFFFF);
  v[1] = (int16_t)(c.x >> 16);
  v[2] = (int16_t)(c.y & 0xFFFF);
  v[3] = (int16_t)(c.y >> 16);
  v[4] = (int16_t)(c.z & 0xFFFF);
  v[5] = (int16_t)(c.z >> 16);
  v[6] = (int16_t)(c.w & 0xFFFF);
}

// The 7 states as a 16-byte cell (the pad half zero).
__device__ __forceinline__ uint4 pack7(const int32_t (&S)[7]) {
  auto pk = [](int32_t lo, int32_t hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16); };
  return make_uint4(pk(S[0], S[1]), pk(S[2], S[3]), pk(S[4], S[5]), pk(S[6], 0));
}

// Literal MAX7 of one target: max_s wrap(pred[s] - pen[s] + add). With TB,
// arg receives the lowest source index achieving it.
template <int T, bool TB>
__device__ __forceinline__ int32_t max7_literal(const int32_t (&pr)[7], const KParams &kp,
                                               int32_t add, int32_t sh, uint32_t &arg) {
  int32_t m = wrapv(pr[0] - kp.pen[T][0] + add, sh);
  uint32_t a = 0;
#pragma unroll
  for (int s = 1; s < 7; ++s) {
    const int32_t v = wrapv(pr[s] - kp.pen[T][s] + add, sh);
    if constexpr (TB) {
      if (v > m) a = s;
    }
    m = max(m, v);
  }
  arg = a;
  return m;
}

// The pair and triple scores of symbols (a, b, cc) (src/PE_1cyc.v:159-162).
__device__ __forceinline__ void literal_adds(const KParams &kp, int a, int b, int cc, int32_t sh,
                                             int32_t &sab, int32_t &sbc, int32_t &sac, int32_t &s3) {
  sab = (a == b) ? kp.match : kp.mismatch;
  sbc = (b == cc) ? kp.match : kp.mismatch;
  sac = (a == cc) ? kp.match : kp.mismatch;
  if (kp.s3_mode == TSA_S3_SOP) s3 = wrapv(sab + sbc + sac, sh);
  else s3 = (a == b) ? ((b == cc) ? kp.s3_eq : kp.s3_ab) : kp.s3_ne;
}

// The traceback cell: the 7 states S of a cell from its 7 predecessor cells
// (literal int32 candidates) and the pointer word, 3 bits per target state =
// the lowest source state that won its MAX7.
__device__ __forceinline__ uint32_t literal_cell_tb(uint4 cM, uint4 cX, uint4 cY, uint4 cZ, uint4 cXY,
                                                    uint4 cYZ, uint4 cXZ, const KParams &kp, int32_t s3,
                                                    int32_t sab, int32_t sbc, int32_t sac, int32_t sh,
                                                    int32_t (&S)[7]) {
  uint32_t g[7];
  int32_t pM[7], pX[7], pY[7], pZ[7], pXY[7], pYZ[7], pXZ[7];
  unpack7(cM, pM);
  unpack7(cX, pX);
  unpack7(cY, pY);
  unpack7(cZ, pZ);
  unpack7(cXY, pXY);
  unpack7(cYZ, pYZ);
  unpack7(cXZ, pXZ);
  S[SM] = max7_literal<SM, true>(pM, kp, s3, sh, g[SM]);
  S[SIX] = max7_literal<SIX, true>(pX, kp, 0, sh, g[SIX]);
  S[SIY] = max7_literal<SIY, true>(pY, kp, 0, sh, g[SIY]);
  S[SIZ] = max7_literal<SIZ, true>(pZ, kp, 0, sh, g[SIZ]);
  S[SIXY] = max7_literal<SIXY, true>(pXY, kp, sab, sh, g[SIXY]);
  S[SIYZ] = max7_literal<SIYZ, true>(pYZ, kp, sbc, sh, g[SIYZ]);
  S[SIXZ] = max7_literal<SIXZ, true>(pXZ, kp, sac, sh, g[SIXZ]);
  uint32_t w = 0;
#pragma unroll
  for (int s = 0; s < NSTATE; ++s) w |= g[s] << (3 * s);
  return w;
}

// Traceback pointer cube index of cell (x,y,z), 1-based: [y-1][x+z-2][z-1].
__host__ __device__ inline int64_t tb_index(int32_t x, int32_t y, int32_t z, int32_t la,
                                            int32_t lc) {
  return ((int64_t)(y - 1) * (la + lc - 1) + (x + z - 2)) * lc + (z - 1);
}

}  // namespace tsa
