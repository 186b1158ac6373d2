// align_tiled_kernel.hip -- the tiled resident traceback kernel of
// tsa_align_batch: one workgroup sweeps a whole (la,lb,lc) cube whose (y,z)
// plane is larger than a workgroup holds, tile by tile, in one launch.
//
// Reference: a (y,z) plane larger than the PE array is sliced into pencils
// swept one after another and chained through face SRAMs
// (src/TriAlign_1cyc.v:78-98,127-140); the cell is that of align_kernel.hip
// (src/PE_1cyc.v:159-218, MAX7 src/PE_1cyc.v:1-32, final MAX7
// src/TriAlign_1cyc.v:141-142), literal_cell.h's max7_literal on the same
// operands. Traceback itself is an extension (src/TriAlign_tb.sv:239-260).
//
// Schedule (tools/align_tiled_emu.py replays it on the CPU). The plane is cut
// into nty x ntz balanced tiles of at most TY x TZ positions
// (align_tile_geom); the workgroup of a triple sweeps them ty outer, tz inner,
// so tiles (ty-1,tz), (ty,tz-1) and (ty-1,tz-1) are finished when (ty,tz)
// starts. A tile is swept over all x by the resident schedule of
// align_kernel.hip in local coordinates, through the same step (align_step.h).
// What differs is what row 0 and column 0 of the buffers hold. In the first
// tile row / column they are the zero faces and nothing is published. In every
// other tile the face position (0,z) is at x = q-z, (y,0) at x = q-y and the
// corner (0,0) at x = q, and while 1 <= x <= la it publishes into buf[q&1] the
// cell the neighbouring tile stored for that (x, global y, global z): the
// rule a real position follows, with a load in place of the cell. (The corner
// publishes x = 1 at step 1, one step before the first real read.) The packed
// cell of a position of a tile's last local row goes into the y face
// [x][global z], that of the last local column into the z face [x][local y];
// the face threads copy it from buf[(q-1)&1] one step after it was published,
// so the cell's own registers carry no face work.
// The y face alternates between two buffers by the parity of ty -- tile
// (ty,tz+1) reads its corner, global z0 of row ty-1, after (ty,tz) has
// written row ty -- and the z face by the parity of tz. Both LDS buffers are
// zeroed and the history reset at the start of every tile, so no cell of the
// last tile reads as a face and the x = 0 face is zero for every tile.
//
// Ordering: face stores and face loads are plain global accesses by threads of
// one workgroup, a tile apart, so at least the end-of-tile __syncthreads()
// lies between them (workgroup scope on one CU). No workgroup waits for
// another: there is no flag, fence or poll.

#include "align_kernel.h"
#include "align_step.h"
#include "pencil_common.h"

namespace tsa {

constexpr int TILED_NT = 1024;  // threads of a workgroup at most
constexpr int TILED_K = 3;      // positions per thread at most: 126 VGPRs of the 128; a fourth would spill

bool align_tile_fits(int32_t ty, int32_t tz) {
  return ty >= 1 && tz >= 1 && (int64_t)ty * tz <= (int64_t)TILED_NT * TILED_K && align_resident_fits(1, ty, tz);
}

// END = TSA_END_FACE / TSA_END_ANY (tsa_align_batch_ends): as the resident
// kernel's, the running best end key of a thread kept across the tiles.
template <int K, int END = TSA_END_CORNER>
__global__ __launch_bounds__(TILED_NT) void align_tiled_kernel(
    const uint8_t *__restrict__ seqs, const int64_t *__restrict__ offs, KParams kp, uint32_t lds_bytes,
    int32_t tymax, int32_t tzmax, int32_t *__restrict__ scores, int32_t *__restrict__ final7,
    uint32_t *__restrict__ tb, const int64_t *__restrict__ tb_off, uint4 *faces,
    const int64_t *__restrict__ face_off, int32_t *__restrict__ endrec) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t t = blockIdx.x;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const AlignTileGeom tg = align_tile_geom(lb, lc, tymax, tzmax);
  const int32_t TY = tg.TY, TZ = tg.TZ;
  const int32_t ldz = TZ + 1, ncell = (TY + 1) * ldz;
  const int tid = threadIdx.x, nt = blockDim.x;
  uint4 *buf0 = (uint4 *)smem, *buf1 = buf0 + ncell;
  uint8_t *sym = (uint8_t *)(buf1 + ncell);
  uint8_t *sB = sym, *sC = sym + TY, *sA = sym + TY + TZ;
  const bool a_lds = align_stage_a(sA, 2 * sizeof(uint4) * (size_t)ncell + TY + TZ, lds_bytes, seqs, o0, la, kp.packed,
                                   tid, nt);
  const auto symA = align_sym_a(a_lds, sA, seqs, o0, la, kp);
  // the face workspace of this triple: y faces [2][la][lc+1], z faces [2][la][TY]
  const int64_t ysz = (int64_t)la * (lc + 1), zsz = (int64_t)la * TY;
  uint4 *yf = faces + face_off[t], *zf = yf + 2 * ysz;
  uint32_t *cube = tb + tb_off[t];
  [[maybe_unused]] AlignEnd end;  // the running best of the thread, kept across the tiles
  for (int32_t ty = 0; ty < tg.nty; ++ty)
    for (int32_t tz = 0; tz < tg.ntz; ++tz) {
      const int32_t y0 = ty * TY, z0 = tz * TZ;
      const int32_t tyl = min(TY, lb - y0), tzl = min(TZ, lc - z0);
      // the last step's barrier of the tile before lies behind: zero both
      // buffers again and stage the tile's symbols of B and C
      for (int32_t i = tid; i < 2 * ncell; i += nt) buf0[i] = make_uint4(0u, 0u, 0u, 0u);
      for (int32_t i = tid; i < tyl; i += nt) sB[i] = (uint8_t)tsa_sym(seqs, o1 + y0 + i, kp.packed);
      for (int32_t i = tid; i < tzl; i += nt) sC[i] = (uint8_t)tsa_sym(seqs, o2 + z0 + i, kp.packed);
      __syncthreads();
      // faces this tile reads (null: the zero face) and writes (null: no tile beyond)
      const uint4 *yrd = ty ? yf + ((ty - 1) & 1) * ysz : nullptr;
      const uint4 *zrd = tz ? zf + ((tz - 1) & 1) * zsz : nullptr;
      uint4 *ywr = ty + 1 < tg.nty ? yf + (ty & 1) * ysz : nullptr;
      uint4 *zwr = tz + 1 < tg.ntz ? zf + (tz & 1) * zsz : nullptr;
      // the positions in local y, z; the history starts again
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
        for (int k = 0; k < K; ++k) {
          if constexpr (END == TSA_END_CORNER)
            P(k).step(rd, wr, ldz, q, la, y0, z0, lb, lc, cube, kp, t, scores, final7, symA);
          else
            P(k).template step<true, END>(rd, wr, ldz, q, la, y0, z0, lb, lc, cube, kp, t, scores, final7, symA, lc,
                                          &end);
        }
        // face work, off the cell's registers: f = 0 the corner, 1 .. tzl row 0
        // and the last local row, tzl+1 .. tzl+tyl column 0 and the last local
        // column. A face position publishes its cell of this step; a position of
        // the last row / column hands on what it published last step (x = q-1-y-z,
        // stable in rd), which is why a tile with a face to write runs one step more.
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
  if constexpr (END != TSA_END_CORNER)
    align_end_reduce(end, (uint64_t *)smem, tid, nt, lb, lc, endrec + ALIGN_END_REC * t, scores + t);
}

// One launch for n triples, triple = workgroup, each swept in tiles of at most
// tymax x tzmax (which must pass align_tile_fits). max_pos = the largest
// TY*TZ of the batch's tile geometries and lds = the largest
// align_resident_lds(la, TY, TZ). d_face_off[t] is the cell offset of triple
// t's align_tiled_face_cells in d_faces.
int align_launch_tiled(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                       int64_t max_pos, size_t lds, const KParams &kp, int32_t *d_scores, int32_t *d_final7,
                       uint32_t *d_tb, const int64_t *d_tb_off, void *d_faces, const int64_t *d_face_off,
                       hipStream_t stream, int32_t end_mode, int32_t *d_endrec) {
  if (n <= 0) return TSA_OK;
  if (end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY || (end_mode != TSA_END_CORNER && !d_endrec)) return TSA_EINVAL;
  if (!align_tile_fits(tymax, tzmax) || max_pos < 1 || max_pos > (int64_t)tymax * tzmax || lds > LDS_MAX || !d_tb ||
      !d_tb_off || !d_faces || !d_face_off)
    return TSA_EINVAL;
  const int k = (int)((max_pos + TILED_NT - 1) / TILED_NT);
  const int nt = (int)(((max_pos + k - 1) / k + 63) / 64 * 64);
  auto launch = [&](auto kfn) {
    return launch_with_lds((const void *)kfn, lds, [&] {
             hipLaunchKernelGGL(kfn, dim3(n), dim3(nt), lds, stream, d_seqs, d_offsets, kp, (uint32_t)lds, tymax,
                                tzmax, d_scores, d_final7, d_tb, d_tb_off, (uint4 *)d_faces, d_face_off,
                                d_endrec);
           }) == hipSuccess
               ? TSA_OK
               : TSA_EDEVICE;
  };
  if (end_mode == TSA_END_FACE) {
    if (k == 1) return launch(align_tiled_kernel<1, TSA_END_FACE>);
    if (k == 2) return launch(align_tiled_kernel<2, TSA_END_FACE>);
    return launch(align_tiled_kernel<3, TSA_END_FACE>);
  }
  if (end_mode == TSA_END_ANY) {
    if (k == 1) return launch(align_tiled_kernel<1, TSA_END_ANY>);
    if (k == 2) return launch(align_tiled_kernel<2, TSA_END_ANY>);
    return launch(align_tiled_kernel<3, TSA_END_ANY>);
  }
  if (k == 1) return launch(align_tiled_kernel<1>);
  if (k == 2) return launch(align_tiled_kernel<2>);
  return launch(align_tiled_kernel<3>);
}

}  // namespace tsa
