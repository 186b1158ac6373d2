// align_kernel.hip -- the resident traceback kernel of tsa_align_batch: one
// workgroup sweeps a whole (la,lb,lc) cube in one launch, the predecessor
// planes resident in LDS, and writes the pointer cube tb_walk_batch follows.
//
// Reference: the recurrence is src/PE_1cyc.v:159-218 with MAX7
// src/PE_1cyc.v:1-32, the zero faces src/PE_1cyc.v:164-218 (x = 0) and
// src/TriAlign_1cyc.v:155-182 (y = 0 / z = 0), the final MAX7
// src/TriAlign_1cyc.v:141-142 -- the same literal cell as the plane sweep
// (literal_cell.h). Traceback itself is an extension: the reference's
// alignment-output ports are commented out (src/TriAlign_tb.sv:239-260).
//
// Schedule (tools/align_emu.py replays it on the CPU). Threads own (y,z)
// positions, up to ALIGN_K each. At step q = 2 .. la+lb+lc position (y,z) is at
// x = q-y-z. LDS holds two (y,z) buffers of 16-byte cells, zeroed at the
// start, with a zero row y = 0 and a zero column z = 0 standing for those
// faces. A position publishes its 7 states into buf[q&1] only while its cell
// is real (1 <= x <= la), so a position that has not started reads as the
// x = 0 face with no extra work, and a position past x = la stops publishing:
// no real cell reads its stale entry. While 0 <= x <= la a position reads from
// buf[(q-1)&1] its own entry and the entries (y-1,z) = N1, (y,z-1) = W1,
// (y-1,z-1) = NW1. The 7 predecessor cells of cell x are
//   M <- NW1 of two steps back   Ix <- own   Iy <- N1   Iz <- W1
//   Ixy <- last step's N1        Iyz <- last step's NW1       Ixz <- last step's W1
// (the read at x = 0 is what hands (1,y-1,z-1) to Iyz of x = 1 and M of x = 2).
// A kept cell would cost 4 VGPRs and the four kept cells of a position 16; but
// the symbols of the later cell are known when the read is made (b, c belong
// to the position, a_{x+1} and a_{x+2} are one lookup), so the step that reads
// N1, W1, NW1 evaluates Ixy, Ixz, Iyz of cell x+1 and M of cell x+2 at once --
// the same max7_literal on the same operands, one or two steps early -- and a
// position keeps 5 states and their argmaxes (6 VGPRs) instead. M of x = 1,
// whose predecessor is the corner of the zero faces, is evaluated at x = 0.
// One barrier per step separates step q's reads of buf[(q-1)&1] from step
// q+1's writes to it.

#include "align_kernel.h"
#include "literal_cell.h"
#include "pencil_common.h"

namespace tsa {

constexpr int ALIGN_NT = 1024;  // threads of a workgroup at most
constexpr int ALIGN_K = 4;      // positions per thread at most (115 VGPRs of the 128 a 1024-thread block has)

static size_t align_cells_bytes(int32_t lb, int32_t lc) {
  return 2 * sizeof(uint4) * (size_t)(lb + 1) * (size_t)(lc + 1);
}

bool align_resident_fits(int32_t la, int32_t lb, int32_t lc) {
  (void)la;  // A is staged when it fits and read from global memory when not
  return (int64_t)lb * lc <= (int64_t)ALIGN_NT * ALIGN_K && align_cells_bytes(lb, lc) + lb + lc <= LDS_MAX;
}

size_t align_resident_lds(int32_t la, int32_t lb, int32_t lc) {
  size_t need = align_cells_bytes(lb, lc) + (size_t)lb + lc;
  if (need + (size_t)la <= LDS_MAX) need += la;
  return std::min<size_t>((need + 15) & ~(size_t)15, LDS_MAX);
}

template <int K>
__global__ __launch_bounds__(ALIGN_NT) void align_resident_kernel(
    const uint8_t *__restrict__ seqs, const int64_t *__restrict__ offs, KParams kp, uint32_t lds_bytes,
    int32_t *__restrict__ scores, int32_t *__restrict__ final7, uint32_t *__restrict__ tb,
    const int64_t *__restrict__ tb_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t t = blockIdx.x;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const int32_t ldz = lc + 1, ncell = (lb + 1) * ldz;
  const int tid = threadIdx.x, nt = blockDim.x;
  uint4 *buf0 = (uint4 *)smem, *buf1 = buf0 + ncell;
  uint8_t *sym = (uint8_t *)(buf1 + ncell);
  // A staged only when the launch's LDS has room for it
  const bool a_lds = 2 * sizeof(uint4) * (size_t)ncell + (size_t)lb + lc + la <= lds_bytes;
  const uint8_t *sB = sym, *sC = sym + lb, *sA = sym + lb + lc;
  for (int32_t i = tid; i < 2 * ncell; i += nt) buf0[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int32_t i = tid; i < lb + lc; i += nt) sym[i] = (uint8_t)tsa_sym(seqs, o1 + i, kp.packed);
  if (a_lds)
    for (int32_t i = tid; i < la; i += nt) sym[lb + lc + i] = (uint8_t)tsa_sym(seqs, o0 + i, kp.packed);
  __syncthreads();

  // position k of this thread: y | z << 13 | b << 26 | c << 28 | valid << 30
  uint32_t meta[K], gh[K];                           // gh: the 5 kept argmaxes, 3 bits each
  int32_t hXY[K], hYZ[K], hXZ[K], hM3[K], hM2[K];    // the kept states
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int32_t p = k * nt + tid;
    meta[k] = 0;
    if (p < lb * lc) {
      const int32_t y = p / lc + 1, z = p % lc + 1;
      meta[k] = (uint32_t)y | ((uint32_t)z << 13) | ((uint32_t)sB[y - 1] << 26) | ((uint32_t)sC[z - 1] << 28) |
                (1u << 30);
    }
    gh[k] = 0;
    hXY[k] = hYZ[k] = hXZ[k] = hM3[k] = hM2[k] = 0;
  }
  uint32_t *cube = tb + tb_off[t];
  const int32_t sh = kp.wrap_shift;
  const int32_t qmax = la + lb + lc;
  auto symA = [&](int32_t i) {  // a_{i+1}, the index clamped into the sequence
    i = min(max(i, 0), la - 1);
    return a_lds ? (int)sA[i] : (int)tsa_sym(seqs, o0 + i, kp.packed);
  };
  for (int32_t q = 2; q <= qmax; ++q) {
    const uint4 *rd = (q & 1) ? buf0 : buf1;  // buf[(q-1)&1]
    uint4 *wr = (q & 1) ? buf1 : buf0;        // buf[q&1]
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int32_t y = (int32_t)(meta[k] & 0x1FFFu), z = (int32_t)((meta[k] >> 13) & 0x1FFFu);
      const int32_t x = q - y - z;
      if ((meta[k] >> 30) && x >= 0 && x <= la) {
        const int32_t idx = y * ldz + z;
        const int b = (int)((meta[k] >> 26) & 3u), cc = (int)((meta[k] >> 28) & 3u);
        int32_t pr[7], sab, sbc, sac, s3;
        uint32_t g;
        if (x == 0) {  // M of x = 1 comes from the corner of the zero faces
          const int32_t zero7[7] = {0, 0, 0, 0, 0, 0, 0};
          literal_adds(kp, symA(0), b, cc, sh, sab, sbc, sac, s3);
          hM3[k] = max7_literal<SM, true>(zero7, kp, s3, sh, g);
          gh[k] = (gh[k] & ~(7u << 9)) | (g << 9);
        } else {
          int32_t S[7];
          uint32_t w = (gh[k] & 7u) << (3 * SIXY) | ((gh[k] >> 3) & 7u) << (3 * SIYZ) |
                       ((gh[k] >> 6) & 7u) << (3 * SIXZ) | ((gh[k] >> 9) & 7u) << (3 * SM);
          S[SM] = hM3[k];
          S[SIXY] = hXY[k];
          S[SIYZ] = hYZ[k];
          S[SIXZ] = hXZ[k];
          unpack7(rd[idx], pr);  // own: (x-1, y, z)
          S[SIX] = max7_literal<SIX, true>(pr, kp, 0, sh, g);
          w |= g << (3 * SIX);
          unpack7(rd[idx - ldz], pr);  // N1: (x, y-1, z)
          S[SIY] = max7_literal<SIY, true>(pr, kp, 0, sh, g);
          w |= g << (3 * SIY);
          unpack7(rd[idx - 1], pr);  // W1: (x, y, z-1)
          S[SIZ] = max7_literal<SIZ, true>(pr, kp, 0, sh, g);
          w |= g << (3 * SIZ);
          wr[idx] = pack7(S);
          cube[tb_index(x, y, z, la, lc)] = w;
          if (x == la && y == lb && z == lc) {  // FINAL_MAX, src/TriAlign_1cyc.v:141-142
            int32_t m = S[0];
#pragma unroll
            for (int s = 1; s < NSTATE; ++s) m = max(m, S[s]);
            scores[t] = m;
#pragma unroll
            for (int s = 0; s < NSTATE; ++s) final7[t * NSTATE + s] = S[s];
          }
          hM3[k] = hM2[k];
          gh[k] = (gh[k] & ~(7u << 9)) | (((gh[k] >> 12) & 7u) << 9);
        }
        // what cells x+1 and x+2 take from this step's reads, evaluated now
        uint32_t gn = gh[k] & (7u << 9);
        literal_adds(kp, symA(x), b, cc, sh, sab, sbc, sac, s3);  // a_{x+1}
        unpack7(rd[idx - ldz], pr);  // N1 = (x, y-1, z): Ixy of x+1
        hXY[k] = max7_literal<SIXY, true>(pr, kp, sab, sh, g);
        gn |= g;
        unpack7(rd[idx - 1], pr);  // W1 = (x, y, z-1): Ixz of x+1
        hXZ[k] = max7_literal<SIXZ, true>(pr, kp, sac, sh, g);
        gn |= g << 6;
        unpack7(rd[idx - ldz - 1], pr);  // NW1 = (x+1, y-1, z-1): Iyz of x+1, M of x+2
        hYZ[k] = max7_literal<SIYZ, true>(pr, kp, sbc, sh, g);
        gn |= g << 3;
        literal_adds(kp, symA(x + 1), b, cc, sh, sab, sbc, sac, s3);  // a_{x+2}
        hM2[k] = max7_literal<SM, true>(pr, kp, s3, sh, g);
        gh[k] = gn | (g << 12);
      }
    }
    __syncthreads();
  }
}

// One launch for n triples, triple = workgroup. max_pos = the largest lb*lc of
// the batch and lds = the largest align_resident_lds; every triple must pass
// align_resident_fits. d_tb_off[t] is the word offset of triple t's cube.
int align_launch_resident(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int64_t max_pos, size_t lds,
                          const KParams &kp, int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb,
                          const int64_t *d_tb_off, hipStream_t stream) {
  if (n <= 0) return TSA_OK;
  if (max_pos < 1 || max_pos > (int64_t)ALIGN_NT * ALIGN_K || lds > LDS_MAX || !d_tb || !d_tb_off) return TSA_EINVAL;
  const int k = max_pos <= ALIGN_NT ? 1 : max_pos <= 2 * ALIGN_NT ? 2 : 4;
  const int nt = (int)(((max_pos + k - 1) / k + 63) / 64 * 64);
  auto launch = [&](auto kfn) {
    return launch_with_lds((const void *)kfn, lds, [&] {
             hipLaunchKernelGGL(kfn, dim3(n), dim3(nt), lds, stream, d_seqs, d_offsets, kp, (uint32_t)lds, d_scores,
                                d_final7, d_tb, d_tb_off);
           }) == hipSuccess
               ? TSA_OK
               : TSA_EDEVICE;
  };
  if (k == 1) return launch(align_resident_kernel<1>);
  if (k == 2) return launch(align_resident_kernel<2>);
  return launch(align_resident_kernel<4>);
}

}  // namespace tsa
