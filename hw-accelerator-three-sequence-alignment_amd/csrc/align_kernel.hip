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
// Schedule (tools/align_emu.py replays it on the CPU; the step itself is
// align_step.h's, shared with align_tiled_kernel.hip). Threads own (y,z)
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
#include "align_step.h"
#include "pencil_common.h"

namespace tsa {

constexpr int ALIGN_NT = 1024;  // threads of a workgroup at most
constexpr int ALIGN_K = 4;      // positions per thread at most (115 VGPRs of the 128 a 1024-thread block has)
static_assert((int64_t)ALIGN_NT * ALIGN_K == ALIGN_RESIDENT_POS && LDS_MAX == ALIGN_LDS_BYTES,
              "align_kernel.h's capacity of the resident kernel");

// END = TSA_END_FACE / TSA_END_ANY (tsa_align_batch_ends): every thread keeps
// the best end key of its cells (align_step.h), the workgroup reduces the keys
// after the last step and thread 0 writes the end record tb_walk_ends starts
// from, and the score; final7 is not written.
template <int K, int END = TSA_END_CORNER>
__global__ __launch_bounds__(ALIGN_NT) void align_resident_kernel(
    const uint8_t *__restrict__ seqs, const int64_t *__restrict__ offs, KParams kp, uint32_t lds_bytes,
    int32_t *__restrict__ scores, int32_t *__restrict__ final7, uint32_t *__restrict__ tb,
    const int64_t *__restrict__ tb_off, int32_t *__restrict__ endrec) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t t = blockIdx.x;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const int32_t ldz = lc + 1, ncell = (lb + 1) * ldz;
  const int tid = threadIdx.x, nt = blockDim.x;
  uint4 *buf0 = (uint4 *)smem, *buf1 = buf0 + ncell;
  uint8_t *sym = (uint8_t *)(buf1 + ncell);  // B, C, then A when there is room
  for (int32_t i = tid; i < 2 * ncell; i += nt) buf0[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int32_t i = tid; i < lb + lc; i += nt) sym[i] = (uint8_t)tsa_sym(seqs, o1 + i, kp.packed);
  uint8_t *sA = sym + lb + lc;
  const bool a_lds = align_stage_a(sA, 2 * sizeof(uint4) * (size_t)ncell + lb + lc, lds_bytes, seqs, o0, la, kp.packed,
                                   tid, nt);
  const auto symA = align_sym_a(a_lds, sA, seqs, o0, la, kp);
  __syncthreads();

  uint32_t meta[K], gh[K];
  int32_t hXY[K], hYZ[K], hXZ[K], hM3[K], hM2[K];
  // position k of this thread is number k * nt + tid of the plane
  auto P = [&](int k) { return AlignPos{meta[k], gh[k], hXY[k], hYZ[k], hXZ[k], hM3[k], hM2[k]}; };
#pragma unroll
  for (int k = 0; k < K; ++k) P(k).init(k * nt + tid, lb, lc, sym, sym + lb);
  uint32_t *cube = tb + tb_off[t];
  const int32_t qmax = la + lb + lc;
  if constexpr (END == TSA_END_CORNER) {
    for (int32_t q = 2; q <= qmax; ++q) {
      const uint4 *rd = (q & 1) ? buf0 : buf1;  // buf[(q-1)&1]
      uint4 *wr = (q & 1) ? buf1 : buf0;        // buf[q&1]
#pragma unroll
      for (int k = 0; k < K; ++k)
        P(k).step(rd, wr, ldz, q, la, 0, 0, lb, lc, cube, kp, t, scores, final7, symA);
      __syncthreads();
    }
  } else {
    AlignEnd end;
    for (int32_t q = 2; q <= qmax; ++q) {
      const uint4 *rd = (q & 1) ? buf0 : buf1;
      uint4 *wr = (q & 1) ? buf1 : buf0;
#pragma unroll
      for (int k = 0; k < K; ++k)
        P(k).template step<true, END>(rd, wr, ldz, q, la, 0, 0, lb, lc, cube, kp, t, scores, final7, symA, lc, &end);
      __syncthreads();
    }
    align_end_reduce(end, (uint64_t *)smem, tid, nt, lb, lc, endrec + ALIGN_END_REC * t, scores + t);
  }
}

// One launch for n triples, triple = workgroup. max_pos = the largest lb*lc of
// the batch and lds = the largest align_resident_lds; every triple must pass
// align_resident_fits. d_tb_off[t] is the word offset of triple t's cube.
int align_launch_resident(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int64_t max_pos, size_t lds,
                          const KParams &kp, int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb,
                          const int64_t *d_tb_off, hipStream_t stream, int32_t end_mode, int32_t *d_endrec) {
  if (n <= 0) return TSA_OK;
  if (max_pos < 1 || max_pos > (int64_t)ALIGN_NT * ALIGN_K || lds > LDS_MAX || !d_tb || !d_tb_off) return TSA_EINVAL;
  if (end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY || (end_mode != TSA_END_CORNER && !d_endrec)) return TSA_EINVAL;
  const int k = max_pos <= ALIGN_NT ? 1 : max_pos <= 2 * ALIGN_NT ? 2 : 4;
  const int nt = (int)(((max_pos + k - 1) / k + 63) / 64 * 64);
  auto launch = [&](auto kfn) {
    return launch_with_lds((const void *)kfn, lds, [&] {
             hipLaunchKernelGGL(kfn, dim3(n), dim3(nt), lds, stream, d_seqs, d_offsets, kp, (uint32_t)lds, d_scores,
                                d_final7, d_tb, d_tb_off, d_endrec);
           }) == hipSuccess
               ? TSA_OK
               : TSA_EDEVICE;
  };
  if (end_mode == TSA_END_FACE) {
    if (k == 1) return launch(align_resident_kernel<1, TSA_END_FACE>);
    if (k == 2) return launch(align_resident_kernel<2, TSA_END_FACE>);
    return launch(align_resident_kernel<4, TSA_END_FACE>);
  }
  if (end_mode == TSA_END_ANY) {
    if (k == 1) return launch(align_resident_kernel<1, TSA_END_ANY>);
    if (k == 2) return launch(align_resident_kernel<2, TSA_END_ANY>);
    return launch(align_resident_kernel<4, TSA_END_ANY>);
  }
  if (k == 1) return launch(align_resident_kernel<1>);
  if (k == 2) return launch(align_resident_kernel<2>);
  return launch(align_resident_kernel<4>);
}

}  // namespace tsa
