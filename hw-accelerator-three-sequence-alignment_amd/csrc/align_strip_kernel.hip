// align_strip_kernel.hip -- the strip traceback kernel of tsa_align_batch under
// align_mode = strip (tsa_align_batch_lowmem): a cube too large for one
// workgroup's planes is aligned with pointers for one tile row at a time.
//
// Reference: as align_tiled_kernel.hip's -- pencils chained through face SRAMs
// (src/TriAlign_1cyc.v:78-98,127-140), the cell of src/PE_1cyc.v:159-218 with
// MAX7 src/PE_1cyc.v:1-32 and the final MAX7 src/TriAlign_1cyc.v:141-142.
// Traceback itself is an extension (src/TriAlign_tb.sv:239-260).
//
// A strip is one tile row of the tiled kernel: TY rows of y, all of z and all
// of x, in ntz tiles of align_tile_geom. The y face below a strip, the last
// row of the tile row before, is a complete checkpoint: the cells of strip s
// depend on that strip's symbols and on y face s-1 alone. With every y face
// kept, a strip can be swept again on its own, so the pointer words of one
// strip, TY*(la+lc-1)*lc of them, are all a triple holds at a time
// (tools/align_strip_emu.py replays the schedule on the CPU):
//
//   forward form  sweeps strips 0 .. nty-2 without pointers, argmaxes or score
//                 (AlignPos::step<false>) and stores the y face of strip s into
//                 a buffer of its own, [nty-1][la][lc+1] cells in all;
//   strip form    launch j = 0, 1, .. sweeps strip s = nty-1-j only: it reads y
//                 face s-1 (the zero face when s = 0), writes no y face and
//                 stores the pointer word of (x,y,z) at
//                 tb_index(x, y - s*TY, z, la, lc) of the strip cube. Strip
//                 nty-1 holds (la,lb,lc), so the step writes score and final
//                 states there. tb_walk_strip (plane_kernel.hip) follows the
//                 pointers of the strip after each launch; once its record says
//                 the path has ended, the strips above it are not swept.
//
// Inside a strip everything is the tiled kernel's: a face position publishes a
// loaded cell, the face threads copy one step late, the z faces alternate by
// the parity of tz, both LDS buffers are zeroed and the history reset at every
// tile. One workgroup per triple; no workgroup waits for another: there is no
// flag, fence or poll. Launches of one stream order a strip's sweep, its walk
// and the next sweep, which overwrites the strip cube.

#include "align_kernel.h"
#include "align_step.h"
#include "pencil_common.h"

namespace tsa {

constexpr int STRIP_NT = 1024;  // as the tiled kernel's: align_tile_fits bounds a tile to 3 positions per thread

// FWD: the forward form (j is not read). Otherwise launch j of the strip form;
// walk = the walker records of tb_walk_strip, ALIGN_WALK_REC words a triple.
template <int K, bool FWD>
__global__ __launch_bounds__(STRIP_NT) void align_strip_kernel(
    const uint8_t *__restrict__ seqs, const int64_t *__restrict__ offs, KParams kp, uint32_t lds_bytes,
    int32_t tymax, int32_t tzmax, int32_t j, const int32_t *__restrict__ walk, int32_t *__restrict__ scores,
    int32_t *__restrict__ final7, uint32_t *__restrict__ tb, const int64_t *__restrict__ tb_off, uint4 *faces,
    const int64_t *__restrict__ face_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t t = blockIdx.x;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const AlignTileGeom tg = align_tile_geom(lb, lc, tymax, tzmax);
  // the strips of this launch, [s0, s1): uniform across the workgroup, and an
  // empty range leaves before the first barrier
  const int32_t s0 = FWD ? 0 : tg.nty - 1 - j, s1 = FWD ? tg.nty - 1 : s0 + 1;
  if (s0 < 0 || s1 <= s0) return;
  if (!FWD && j > 0 && walk[ALIGN_WALK_REC * t + 5]) return;  // the path ended in a strip below
  const int32_t TY = tg.TY, TZ = tg.TZ;
  const int32_t ldz = TZ + 1, ncell = (TY + 1) * ldz;
  const int tid = threadIdx.x, nt = blockDim.x;
  uint4 *buf0 = (uint4 *)smem, *buf1 = buf0 + ncell;
  uint8_t *sym = (uint8_t *)(buf1 + ncell);
  uint8_t *sB = sym, *sC = sym + TY, *sA = sym + TY + TZ;
  const bool a_lds = align_stage_a(sA, 2 * sizeof(uint4) * (size_t)ncell + TY + TZ, lds_bytes, seqs, o0, la, kp.packed,
                                   tid, nt);
  const auto symA = align_sym_a(a_lds, sA, seqs, o0, la, kp);
  // the face workspace of this triple: y faces [nty-1][la][lc+1], z faces [2][la][TY]
  const int64_t ysz = (int64_t)la * (lc + 1), zsz = (int64_t)la * TY;
  uint4 *yf = faces + face_off[t], *zf = yf + (tg.nty - 1) * ysz;
  // the strip cube, set back by the rows below the strip: the step indexes it by global y
  uint32_t *cube = FWD ? nullptr : tb + tb_off[t] - (int64_t)s0 * TY * (la + lc - 1) * lc;
  for (int32_t ty = s0; ty < s1; ++ty)
    for (int32_t tz = 0; tz < tg.ntz; ++tz) {
      const int32_t y0 = ty * TY, z0 = tz * TZ;
      const int32_t tyl = min(TY, lb - y0), tzl = min(TZ, lc - z0);
      // the last step's barrier of the tile before lies behind: zero both
      // buffers again and stage the tile's symbols of B and C
      for (int32_t i = tid; i < 2 * ncell; i += nt) buf0[i] = make_uint4(0u, 0u, 0u, 0u);
      for (int32_t i = tid; i < tyl; i += nt) sB[i] = (uint8_t)tsa_sym(seqs, o1 + y0 + i, kp.packed);
      for (int32_t i = tid; i < tzl; i += nt) sC[i] = (uint8_t)tsa_sym(seqs, o2 + z0 + i, kp.packed);
      __syncthreads();
      // faces this tile reads (null: the zero face) and writes (null: none kept)
      const uint4 *yrd = ty ? yf + (ty - 1) * ysz : nullptr;
      const uint4 *zrd = tz ? zf + ((tz - 1) & 1) * zsz : nullptr;
      uint4 *ywr = FWD ? yf + ty * ysz : nullptr;
      uint4 *zwr = tz + 1 < tg.ntz ? zf + (tz & 1) * zsz : nullptr;
      uint32_t meta[K], gh[K];
      int32_t hXY[K], hYZ[K], hXZ[K], hM3[K], hM2[K];
      auto P = [&](int k) { return AlignPos{meta[k], gh[k], hXY[k], hYZ[k], hXZ[k], hM3[k], hM2[k]}; };
#pragma unroll
      for (int k = 0; k < K; ++k) P(k).init(k * nt + tid, tyl, tzl, sB, sC);
      const int32_t qmax = la + tyl + tzl + ((ywr || zwr) ? 1 : 0);
      for (int32_t q = 1; q <= qmax; ++q) {
        const uint4 *rd = (q & 1) ? buf0 : buf1;  // buf[(q-1)&1]
        uint4 *wr = (q & 1) ? buf1 : buf0;        // buf[q&1]
#pragma unroll
        for (int k = 0; k < K; ++k)
          P(k).template step<!FWD>(rd, wr, ldz, q, la, y0, z0, lb, lc, cube, kp, t, scores, final7, symA);
        // the face threads, as the tiled kernel's: f = 0 the corner, 1 .. tzl
        // row 0 and the last local row, tzl+1 .. tzl+tyl column 0 and the last
        // local column
        for (int32_t f = tid; f <= tzl + tyl; f += nt) {
          const bool row = f <= tzl;
          const int32_t y = row ? 0 : f - tzl, z = row ? f : 0;
          const int32_t x = q - y - z;
          const uint4 *src = row ? ((f || zrd) ? yrd : nullptr) : zrd;  // the corner of a first column is zero
          if (src && x >= 1 && x <= la)
            wr[y * ldz + z] = src[row ? (int64_t)(x - 1) * (lc + 1) + z0 + z : (int64_t)(x - 1) * TY + (y - 1)];
          const int32_t sy = row ? tyl : y, sz = row ? z : tzl;
          const int32_t sx = q - 1 - sy - sz;
          uint4 *dst = row ? ywr : zwr;
          if (f && dst && sx >= 1 && sx <= la)
            dst[row ? (int64_t)(sx - 1) * (lc + 1) + z0 + sz : (int64_t)(sx - 1) * TY + (sy - 1)] = rd[sy * ldz + sz];
        }
        __syncthreads();
      }
    }
}

// One launch for n triples, triple = workgroup: j < 0 the forward form,
// j >= 0 launch j of the strip form. The tile caps, max_pos and lds as
// align_launch_tiled's; d_tb_off[t] = the word offset of triple t's strip cube,
// d_face_off[t] = the cell offset of its align_strip_face_cells in d_faces.
int align_launch_strip(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                       int64_t max_pos, size_t lds, const KParams &kp, int32_t j, const int32_t *d_walk,
                       int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb, const int64_t *d_tb_off, void *d_faces,
                       const int64_t *d_face_off, hipStream_t stream) {
  if (n <= 0) return TSA_OK;
  if (!align_tile_fits(tymax, tzmax) || max_pos < 1 || max_pos > (int64_t)tymax * tzmax || lds > LDS_MAX || !d_tb ||
      !d_tb_off || !d_faces || !d_face_off || !d_walk)
    return TSA_EINVAL;
  const int k = (int)((max_pos + STRIP_NT - 1) / STRIP_NT);
  const int nt = (int)(((max_pos + k - 1) / k + 63) / 64 * 64);
  auto launch = [&](auto kfn) {
    return launch_with_lds((const void *)kfn, lds, [&] {
             hipLaunchKernelGGL(kfn, dim3(n), dim3(nt), lds, stream, d_seqs, d_offsets, kp, (uint32_t)lds, tymax,
                                tzmax, j, d_walk, d_scores, d_final7, d_tb, d_tb_off, (uint4 *)d_faces, d_face_off);
           }) == hipSuccess
               ? TSA_OK
               : TSA_EDEVICE;
  };
  if (j < 0) {
    if (k == 1) return launch(align_strip_kernel<1, true>);
    if (k == 2) return launch(align_strip_kernel<2, true>);
    return launch(align_strip_kernel<3, true>);
  }
  if (k == 1) return launch(align_strip_kernel<1, false>);
  if (k == 2) return launch(align_strip_kernel<2, false>);
  return launch(align_strip_kernel<3, false>);
}

}  // namespace tsa
