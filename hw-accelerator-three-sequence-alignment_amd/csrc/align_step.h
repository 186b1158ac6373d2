// align_step.h -- what the resident traceback kernels share: the staging
// and the lookup of A's symbols, the register state of a (y,z) position and
// one step of the schedule for it. align_kernel.hip explains the schedule and
// calls the step with its whole plane as the one tile; align_tiled_kernel.hip
// align_strip_kernel.hip and align_grid_kernel.hip call it tile by tile, the
// forward forms of the latter two without the pointer word. The cell is literal_cell.h's max7_literal on the
// plane sweep's operands (src/PE_1cyc.v:159-218, MAX7 src/PE_1cyc.v:1-32).
//
// Both kernels sit at the SGPR limit, where one more SGPR is a spilled VGPR, and
// this shape is the one that kept their register counts: the
// state in the kernel's own arrays with AlignPos a view of one entry, the loop
// over the positions in the kernel, the A lookup a closure over its variables.
#pragma once

#include <type_traits>

#include "align_kernel.h"
#include "literal_cell.h"

namespace tsa {

// A staged at sA, behind `used` bytes of the launch's lds_bytes of LDS, only
// when there is room for it: true when it was. The caller's next barrier
// orders the stores before the first lookup.
__device__ __forceinline__ bool align_stage_a(uint8_t *sA, size_t used, uint32_t lds_bytes, const uint8_t *seqs,
                                              int64_t o0, int32_t la, int32_t packed, int tid, int nt) {
  const bool room = used + (size_t)la <= lds_bytes;
  if (room)
    for (int32_t i = tid; i < la; i += nt) sA[i] = (uint8_t)tsa_sym(seqs, o0 + i, packed);
  return room;
}

// The lookup of a_{i+1}, the index clamped into the sequence: from LDS (sA)
// when A was staged there, from global memory when not. A closure over the
// caller's own variables (lvalues only), which must outlive it.
template <class L, class PA, class PS, class O, class N>
__device__ __forceinline__ auto align_sym_a(L &&lds, PA &&sA, PS &&seqs, O &&o0, N &&la, const KParams &kp) {
  static_assert(std::is_lvalue_reference_v<L> && std::is_lvalue_reference_v<PA> && std::is_lvalue_reference_v<PS> &&
                std::is_lvalue_reference_v<O> && std::is_lvalue_reference_v<N>, "align_sym_a keeps references");
  return [&](int32_t i) {
    i = min(max(i, 0), la - 1);
    return lds ? (int)sA[i] : (int)tsa_sym(seqs, o0 + i, kp.packed);
  };
}

// The end search of tsa_align_batch_ends (TSA_END_FACE, TSA_END_ANY): the
// candidate cell whose MAX7 is largest ends the path; ties go to the smallest
// x, then y, then z, and to the lowest state. One totally ordered 64-bit key
// says all of it, so a plain max over the cells in any order is the rule:
//   [63:48] MAX7 + 32768 (a state is an int16, pack7)
//   [47:3]  ~pos, pos = ((x-1)*lb + (y-1))*lc + (z-1) < la*lb*lc, the cell's
//           number in (x,y,z) order: no width to carry but lb and lc, which the
//           kernels hold anyway. A pointer cube has more words than that, so
//           every cube that fits device memory fits the 45 bits
//           (align_end_key_fits).
//   [2:0]   7 - the lowest state that reaches the MAX7
// The running best of a thread, across its positions and tiles; 0 = none yet.
struct AlignEnd {
  uint64_t best = 0;
  __device__ __forceinline__ void fold(const int32_t (&S)[7], int32_t x, int32_t y, int32_t z, int32_t lb,
                                       int32_t lc) {
    // Nothing of the key is to be hoisted out of the step loop into registers
    // of its own (the cell's number less its x term is invariant there): that
    // alone spilled the widest instantiations.
    asm volatile("" : "+v"(y), "+v"(z));
    int32_t m = S[0] * 8 + 7;  // the max of (state value, 7 - index) pairs: the lowest index of the largest value
#pragma unroll
    for (int s = 1; s < NSTATE; ++s) m = max(m, S[s] * 8 + (7 - s));
    const uint64_t pos = ((uint64_t)(uint32_t)(x - 1) * (uint32_t)lb + (uint32_t)(y - 1)) * (uint32_t)lc +
                         (uint32_t)(z - 1);
    const uint64_t key = ((uint64_t)(uint32_t)((m >> 3) + 32768) << 48) | ((~pos & ALIGN_END_POS_MASK) << 3) |
                         (uint32_t)(m & 7);
    best = max(best, key);
  }
};

// A key back into the end record rec = {x1, y1, z1, state, score} of a cube
// whose rows are lc long and whose planes have lb rows.
__device__ __forceinline__ void align_end_decode(uint64_t k, int32_t lb, int32_t lc, int32_t *rec) {
  const uint64_t pos = ~(k >> 3) & ALIGN_END_POS_MASK, row = pos / (uint32_t)lc;
  rec[0] = (int32_t)(row / (uint32_t)lb) + 1;
  rec[1] = (int32_t)(row % (uint32_t)lb) + 1;
  rec[2] = (int32_t)(pos % (uint32_t)lc) + 1;
  rec[3] = 7 - (int32_t)(k & 7u);
  rec[4] = (int32_t)(k >> 48) - 32768;
}

// The workgroup's best key after its last step (whose barrier lies behind, so
// slots, LDS for one key per wave, may be the cell buffers): a wave reduce,
// then thread 0 over the waves' keys. The return value is the workgroup's key
// in thread 0 alone.
__device__ __forceinline__ uint64_t align_end_reduce_key(const AlignEnd &end, uint64_t *slots, int tid, int nt) {
  uint64_t k = end.best;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)k, d, 64), hi = __shfl_xor((uint32_t)(k >> 32), d, 64);
    k = max(k, ((uint64_t)hi << 32) | lo);
  }
  if ((tid & 63) == 0) slots[tid >> 6] = k;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < nt / 64; ++w) k = max(k, slots[w]);
  return k;
}

// A workgroup that has swept the whole cube: thread 0 writes the triple's end
// record and its score.
__device__ __forceinline__ void align_end_reduce(const AlignEnd &end, uint64_t *slots, int tid, int nt, int32_t lb,
                                                 int32_t lc, int32_t *rec, int32_t *score) {
  const uint64_t k = align_end_reduce_key(end, slots, tid, nt);
  if (tid == 0) {
    align_end_decode(k, lb, lc, rec);
    *score = rec[4];
  }
}

// One (y,z) position of a thread, in the coordinates of its tile: a view of
// entry k of the kernel's arrays
//   uint32_t meta[K], gh[K];  int32_t hXY[K], hYZ[K], hXZ[K], hM3[K], hM2[K];
struct AlignPos {
  uint32_t &meta;  // y | z << 13 | b << 26 | c << 28 | valid << 30
  uint32_t &gh;    // the 5 kept argmaxes, 3 bits each
  int32_t &hXY, &hYZ, &hXZ, &hM3, &hM2;  // the kept states

  // Position number p of a tyl x tzl tile, row by row from (1,1) (none when p
  // is past the tile); sB, sC: the tile's symbols of B and C. The history is zero.
  __device__ __forceinline__ void init(int32_t p, int32_t tyl, int32_t tzl, const uint8_t *sB, const uint8_t *sC) {
    meta = 0;
    if (p < tyl * tzl) {
      const int32_t y = p / tzl + 1, z = p % tzl + 1;
      meta = (uint32_t)y | ((uint32_t)z << 13) | ((uint32_t)sB[y - 1] << 26) | ((uint32_t)sC[z - 1] << 28) | (1u << 30);
    }
    gh = 0;
    hXY = hYZ = hXZ = hM3 = hM2 = 0;
  }

  // Step q of a tile whose local (0,0) is global (y0,z0): the position, while
  // 0 <= x = q-y-z <= la reads rd = buf[(q-1)&1] (row stride ldz) and, while
  // x >= 1, publishes its cell into wr = buf[q&1], stores its pointer word in
  // cube and, at the cube's end (la,lb,lc), the triple's score and final states.
  // TB = false (the forward forms of align_strip_kernel.hip and
  // align_grid_kernel.hip): the cells alone, no argmax, no pointer word, no
  // score. cld: the words of a row of the cube, tb_index's lc -- lc itself
  // unless the cube holds one tile (align_grid_kernel.hip).
  template <bool TB = true, class SymA>
  __device__ __forceinline__ void step(const uint4 *rd, uint4 *wr, int32_t ldz, int32_t q, int32_t la, int32_t y0,
                                       int32_t z0, int32_t lb, int32_t lc, uint32_t *cube, const KParams &kp,
                                       int64_t t, int32_t *scores, int32_t *final7, const SymA &symA) {
    step<TB>(rd, wr, ldz, q, la, y0, z0, lb, lc, cube, kp, t, scores, final7, symA, lc);
  }
  // END = TSA_END_FACE / TSA_END_ANY (the kernels of tsa_align_batch_ends):
  // a cell that may end the path also folds its end key into the thread's
  // running best `end`, and the corner gives no score and no final states --
  // the reduction of the keys does (align_end_reduce). With TB = false (the
  // forward END form of align_grid_kernel.hip) the fold is all that is added.
  // END = ALIGN_END_PTRS (its backward END form, TB = true): the pointer word
  // alone, no fold and nothing at the corner -- the end is known by then, and
  // the swept range may hold (la,lb,lc) without the path ending there.
  template <bool TB = true, int END = 0, class SymA>
  __device__ __forceinline__ void step(const uint4 *rd, uint4 *wr, int32_t ldz, int32_t q, int32_t la, int32_t y0,
                                       int32_t z0, int32_t lb, int32_t lc, uint32_t *cube, const KParams &kp,
                                       int64_t t, int32_t *scores, int32_t *final7, const SymA &symA, int32_t cld,
                                       AlignEnd *end = nullptr) {
    const int32_t sh = kp.wrap_shift;
    const int32_t y = (int32_t)(meta & 0x1FFFu), z = (int32_t)((meta >> 13) & 0x1FFFu);
    const int32_t x = q - y - z;
    if ((meta >> 30) && x >= 0 && x <= la) {
      const int32_t idx = y * ldz + z;
      const int b = (int)((meta >> 26) & 3u), cc = (int)((meta >> 28) & 3u);
      int32_t pr[7], sab, sbc, sac, s3;
      uint32_t g;
      if (x == 0) {  // M of x = 1 comes from the corner of the zero faces
        const int32_t zero7[7] = {0, 0, 0, 0, 0, 0, 0};
        literal_adds(kp, symA(0), b, cc, sh, sab, sbc, sac, s3);
        hM3 = max7_literal<SM, TB>(zero7, kp, s3, sh, g);
        gh = (gh & ~(7u << 9)) | (g << 9);
      } else {
        int32_t S[7];
        uint32_t w = (gh & 7u) << (3 * SIXY) | ((gh >> 3) & 7u) << (3 * SIYZ) |
                     ((gh >> 6) & 7u) << (3 * SIXZ) | ((gh >> 9) & 7u) << (3 * SM);
        S[SM] = hM3;
        S[SIXY] = hXY;
        S[SIYZ] = hYZ;
        S[SIXZ] = hXZ;
        unpack7(rd[idx], pr);  // own: (x-1, y, z)
        S[SIX] = max7_literal<SIX, TB>(pr, kp, 0, sh, g);
        w |= g << (3 * SIX);
        unpack7(rd[idx - ldz], pr);  // N1: (x, y-1, z)
        S[SIY] = max7_literal<SIY, TB>(pr, kp, 0, sh, g);
        w |= g << (3 * SIY);
        unpack7(rd[idx - 1], pr);  // W1: (x, y, z-1)
        S[SIZ] = max7_literal<SIZ, TB>(pr, kp, 0, sh, g);
        w |= g << (3 * SIZ);
        wr[idx] = pack7(S);
        if constexpr (TB) cube[tb_index(x, y0 + y, z0 + z, la, cld)] = w;
        if constexpr (END > 0) {  // with or without pointers: the key is the cell's values alone
          if (END == TSA_END_ANY || x == la || y0 + y == lb || z0 + z == lc) end->fold(S, x, y0 + y, z0 + z, lb, lc);
        } else if constexpr (TB && END == 0) {
          if (x == la && y0 + y == lb && z0 + z == lc) {  // FINAL_MAX, src/TriAlign_1cyc.v:141-142
            int32_t m = S[0];
#pragma unroll
            for (int s = 1; s < NSTATE; ++s) m = max(m, S[s]);
            scores[t] = m;
#pragma unroll
            for (int s = 0; s < NSTATE; ++s) final7[t * NSTATE + s] = S[s];
          }
        }
        hM3 = hM2;
        gh = (gh & ~(7u << 9)) | (((gh >> 12) & 7u) << 9);
      }
      // what cells x+1 and x+2 take from this step's reads, evaluated now
      uint32_t gn = gh & (7u << 9);
      literal_adds(kp, symA(x), b, cc, sh, sab, sbc, sac, s3);  // a_{x+1}
      unpack7(rd[idx - ldz], pr);  // N1 = (x, y-1, z): Ixy of x+1
      hXY = max7_literal<SIXY, TB>(pr, kp, sab, sh, g);
      gn |= g;
      unpack7(rd[idx - 1], pr);  // W1 = (x, y, z-1): Ixz of x+1
      hXZ = max7_literal<SIXZ, TB>(pr, kp, sac, sh, g);
      gn |= g << 6;
      unpack7(rd[idx - ldz - 1], pr);  // NW1 = (x+1, y-1, z-1): Iyz of x+1, M of x+2
      hYZ = max7_literal<SIYZ, TB>(pr, kp, sbc, sh, g);
      gn |= g << 3;
      literal_adds(kp, symA(x + 1), b, cc, sh, sab, sbc, sac, s3);  // a_{x+2}
      hM2 = max7_literal<SM, TB>(pr, kp, s3, sh, g);
      gh = gn | (g << 12);
    }
  }
};

}  // namespace tsa
