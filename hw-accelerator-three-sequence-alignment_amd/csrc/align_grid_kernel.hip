// align_grid_kernel.hip -- the grid traceback kernels of tsa_align_batch under
// align_mode = grid (tsa_align_batch_grid): every tile of a cube too large for
// one workgroup is checkpointed, the tiles of one anti-diagonal of the tile grid
// are swept by separate workgroups, and only the tiles on the path are swept
// again with pointers.
//
// Reference: as align_tiled_kernel.hip's -- pencils chained through face SRAMs
// (src/TriAlign_1cyc.v:78-98,127-140), the cell of src/PE_1cyc.v:159-218 with
// MAX7 src/PE_1cyc.v:1-32 and the final MAX7 src/TriAlign_1cyc.v:141-142.
// Traceback itself is an extension (src/TriAlign_tb.sv:239-260).
//
// The tiles are the tiled kernel's (align_tile_geom). The cells of tile (ty,tz)
// depend on the tile's symbols, on the last row of tile row ty-1 (the y face)
// and on the last column of tile column tz-1 (the z face) alone. With both
// faces of every tile kept, [nty-1][la][lc+1] and [ntz-1][la][lb] cells, any
// tile can be swept again on its own, so the pointer words of one tile,
// TY*(la+TZ-1)*TZ of them, are all a triple holds at a time
// (tools/align_grid_emu.py replays the schedule on the CPU):
//
//   forward form   launch d = 0 .. nty+ntz-3 sweeps every tile with ty+tz = d,
//                  one workgroup each (blockIdx.y = the index along the
//                  diagonal), without pointers, argmaxes or score
//                  (AlignPos::step<false>). A tile stores its y face unless
//                  ty = nty-1 and its z face unless tz = ntz-1; the last tile
//                  (nty-1,ntz-1) stores neither and is not swept here.
//   backward form  launch j = 0, 1, .. sweeps, one workgroup per triple, the
//                  tile that holds the cell of the triple's walker record
//                  (tile (nty-1,ntz-1) when j = 0), and of it only the cells
//                  with x <= the record's x = xm: a move never increases x, so
//                  no later cell can lie on the path. It writes no face and
//                  stores the pointer word of (x,y,z) at
//                  tb_index(x, y - y0, z - z0, xm, TZ) of the tile cube. Launch
//                  0 has xm = la and holds (la,lb,lc), so the step writes score
//                  and final states there. tb_walk_grid (plane_kernel.hip)
//                  follows the pointers after each launch; a triple whose
//                  record says the path has ended is not swept again.
//
// The tiles of one diagonal write disjoint face regions -- tile (ty,tz) the
// columns z0+1 .. z0+tzl of y face ty and the rows y0+1 .. y0+tyl of z face tz
// -- and read only what earlier launches wrote: y face ty-1 at z0 .. z0+tzl (the
// corner z0 from tile (ty-1,tz-1), two diagonals back) and z face tz-1. Inside a
// tile everything is the tiled kernel's: a face position publishes a loaded
// cell, the face threads copy one step late. No workgroup waits for another:
// there is no flag, fence or poll. Launches of one stream order the diagonals,
// a tile's sweep, its walk and the next sweep, which overwrites the tile cube.
//
// The END forms (tsa_align_batch_grid_ends under TSA_END_FACE / TSA_END_ANY)
// search the cell the path ends in as the resident kernels do, by align_step.h's
// 64-bit key:
//
//   forward END    launch d = 0 .. nty+ntz-2 sweeps every tile, the last one
//                  included (it stores no face), and every cell that may end
//                  the path folds its key into the thread's running best. After
//                  its last step the workgroup reduces its keys and thread 0
//                  stores the tile's key into the slot ty*ntz+tz of the triple's
//                  nty*ntz slots. Every tile writes its slot in every call, so
//                  the slots are never cleared, and a plain max has no order, so
//                  no atomics either.
//   end record     align_grid_end_kernel, one thread per triple, takes the max
//                  over the slots and writes the score, the end record
//                  {x1, y1, z1, state, score} and the walker record
//                  {x1, y1, z1, state, 0, 0}.
//   backward END   launch 0 reads the walker record like every later launch:
//                  the tile of (y1,z1), x <= x1. Its step stores pointer words
//                  alone (ALIGN_END_PTRS): when the end lies in the last tile
//                  with x1 = la the swept cells hold (la,lb,lc), and the corner's
//                  score and final states would overwrite the end's score and
//                  the end record, which lies on final7. tb_walk_grid is
//                  launched with j + 1, so it takes cell and state from the
//                  record from the first segment on.

#include "align_kernel.h"
#include "align_step.h"
#include "pencil_common.h"

namespace tsa {

constexpr int GRID_NT = 1024;  // as the tiled kernel's: align_tile_fits bounds a tile to 3 positions per thread

// FWD: launch d of the forward form (walk is not read). Otherwise launch d of
// the backward form; walk = the walker records of tb_walk_grid, ALIGN_WALK_REC
// words a triple.
// END = TSA_END_FACE / TSA_END_ANY: the forward END form, where tb and tb_off
// are not the cubes' but the key slots' -- (uint64_t *)tb + tb_off[t] = the
// nty*ntz slots of triple t -- or, for any END != 0, the backward END form.
template <int K, bool FWD, int END = TSA_END_CORNER>
__global__ __launch_bounds__(GRID_NT) void align_grid_kernel(
    const uint8_t *__restrict__ seqs, const int64_t *__restrict__ offs, KParams kp, uint32_t lds_bytes,
    int32_t tymax, int32_t tzmax, int32_t d, const int32_t *__restrict__ walk, int32_t *__restrict__ scores,
    int32_t *__restrict__ final7, uint32_t *__restrict__ tb, const int64_t *__restrict__ tb_off, uint4 *faces,
    const int64_t *__restrict__ face_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int64_t t = blockIdx.x;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const AlignTileGeom tg = align_tile_geom(lb, lc, tymax, tzmax);
  const int32_t TY = tg.TY, TZ = tg.TZ;
  // the tile of this workgroup and the x it sweeps up to: uniform across the
  // workgroup, and one with no tile leaves before the first barrier
  int32_t ty, tz, xm = la;
  if (FWD) {
    ty = max(0, d - (tg.ntz - 1)) + (int32_t)blockIdx.y;
    tz = d - ty;
    if (ty >= tg.nty || tz < 0 || (END == TSA_END_CORNER && ty == tg.nty - 1 && tz == tg.ntz - 1))
      return;
  } else if (END == TSA_END_CORNER && d == 0) {
    ty = tg.nty - 1, tz = tg.ntz - 1;
  } else {
    const int32_t *rec = walk + ALIGN_WALK_REC * t;
    if (rec[5]) return;  // the path has ended
    xm = rec[0], ty = (rec[1] - 1) / TY, tz = (rec[2] - 1) / TZ;
  }
  const int32_t ldz = TZ + 1, ncell = (TY + 1) * ldz;
  const int tid = threadIdx.x, nt = blockDim.x;
  uint4 *buf0 = (uint4 *)smem, *buf1 = buf0 + ncell;
  uint8_t *sym = (uint8_t *)(buf1 + ncell);
  uint8_t *sB = sym, *sC = sym + TY, *sA = sym + TY + TZ;
  const bool a_lds = align_stage_a(sA, 2 * sizeof(uint4) * (size_t)ncell + TY + TZ, lds_bytes, seqs, o0, la, kp.packed,
                                   tid, nt);
  const auto symA = align_sym_a(a_lds, sA, seqs, o0, la, kp);
  const int32_t y0 = ty * TY, z0 = tz * TZ;
  const int32_t tyl = min(TY, lb - y0), tzl = min(TZ, lc - z0);
  for (int32_t i = tid; i < 2 * ncell; i += nt) buf0[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int32_t i = tid; i < tyl; i += nt) sB[i] = (uint8_t)tsa_sym(seqs, o1 + y0 + i, kp.packed);
  for (int32_t i = tid; i < tzl; i += nt) sC[i] = (uint8_t)tsa_sym(seqs, o2 + z0 + i, kp.packed);
  __syncthreads();
  // the kept faces of this triple: y faces [nty-1][la][lc+1], z faces [ntz-1][la][lb]
  const int64_t ysz = (int64_t)la * (lc + 1), zsz = (int64_t)la * lb;
  uint4 *yf = faces + face_off[t], *zf = yf + (tg.nty - 1) * ysz;
  // faces this tile reads (null: the zero face) and writes (null: none kept)
  const uint4 *yrd = ty ? yf + (ty - 1) * ysz : nullptr;
  const uint4 *zrd = tz ? zf + (tz - 1) * zsz : nullptr;
  uint4 *ywr = FWD && ty + 1 < tg.nty ? yf + ty * ysz : nullptr;
  uint4 *zwr = FWD && tz + 1 < tg.ntz ? zf + tz * zsz : nullptr;
  // the tile cube, rows of TZ words over xm planes, set back by the rows and
  // columns before the tile: the step indexes it by global y and z
  uint32_t *cube = FWD ? nullptr : tb + tb_off[t] - ((int64_t)y0 * (xm + TZ - 1) * TZ + (int64_t)z0 * (TZ + 1));
  uint32_t meta[K], gh[K];
  int32_t hXY[K], hYZ[K], hXZ[K], hM3[K], hM2[K];
  auto P = [&](int k) { return AlignPos{meta[k], gh[k], hXY[k], hYZ[k], hXZ[k], hM3[k], hM2[k]}; };
  [[maybe_unused]] AlignEnd end;  // the running best of the thread (forward END form)
#pragma unroll
  for (int k = 0; k < K; ++k) P(k).init(k * nt + tid, tyl, tzl, sB, sC);
  const int32_t qmax = xm + tyl + tzl + ((ywr || zwr) ? 1 : 0);
  for (int32_t q = 1; q <= qmax; ++q) {
    const uint4 *rd = (q & 1) ? buf0 : buf1;  // buf[(q-1)&1]
    uint4 *wr = (q & 1) ? buf1 : buf0;        // buf[q&1]
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr (END == TSA_END_CORNER)
        P(k).template step<!FWD>(rd, wr, ldz, q, xm, y0, z0, lb, lc, cube, kp, t, scores, final7, symA, TZ);
      else if constexpr (FWD)
        P(k).template step<false, END>(rd, wr, ldz, q, xm, y0, z0, lb, lc, cube, kp, t, scores, final7, symA, TZ,
                                       &end);
      else
        P(k).template step<true, ALIGN_END_PTRS>(rd, wr, ldz, q, xm, y0, z0, lb, lc, cube, kp, t, scores, final7,
                                                 symA, TZ);
    }
    // the face threads, as the tiled kernel's: f = 0 the corner, 1 .. tzl
    // row 0 and the last local row, tzl+1 .. tzl+tyl column 0 and the last
    // local column
    for (int32_t f = tid; f <= tzl + tyl; f += nt) {
      const bool row = f <= tzl;
      const int32_t y = row ? 0 : f - tzl, z = row ? f : 0;
      const int32_t x = q - y - z;
      const uint4 *src = row ? ((f || zrd) ? yrd : nullptr) : zrd;  // the corner of a first column is zero
      if (src && x >= 1 && x <= xm)
        wr[y * ldz + z] = src[row ? (int64_t)(x - 1) * (lc + 1) + z0 + z : (int64_t)(x - 1) * lb + y0 + (y - 1)];
      const int32_t sy = row ? tyl : y, sz = row ? z : tzl;
      const int32_t sx = q - 1 - sy - sz;
      uint4 *dst = row ? ywr : zwr;
      if (f && dst && sx >= 1 && sx <= xm)
        dst[row ? (int64_t)(sx - 1) * (lc + 1) + z0 + sz : (int64_t)(sx - 1) * lb + y0 + (sy - 1)] = rd[sy * ldz + sz];
    }
    __syncthreads();
  }
  if constexpr (FWD && END != TSA_END_CORNER) {
    const uint64_t key = align_end_reduce_key(end, (uint64_t *)smem, tid, nt);
    if (tid == 0) ((uint64_t *)tb)[tb_off[t] + (int64_t)ty * tg.ntz + tz] = key;
  }
}

// The end record of every grid triple from the keys of its tiles, one thread
// per triple: the largest key decoded into endrec[5t ..] and scores[t], and the
// walker record {x1, y1, z1, state, 0, 0} the backward END form starts from. A
// key that names no cell of the cube (0: no slot written) ends the triple at
// once with info[4t] = 0 moves, which the host reports as TSA_EINTERNAL.
__global__ __launch_bounds__(64) void align_grid_end_kernel(const int64_t *__restrict__ offs, int32_t n, int32_t tymax,
                                                            int32_t tzmax, const uint64_t *__restrict__ slots,
                                                            const int64_t *__restrict__ slot_off,
                                                            int32_t *__restrict__ scores, int32_t *__restrict__ endrec,
                                                            int32_t *__restrict__ walk, int32_t *__restrict__ info) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t o0 = offs[3 * t], o1 = offs[3 * t + 1], o2 = offs[3 * t + 2], o3 = offs[3 * t + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const AlignTileGeom tg = align_tile_geom(lb, lc, tymax, tzmax);
  const uint64_t *s = slots + slot_off[t];
  uint64_t k = 0;
  for (int32_t i = 0; i < tg.nty * tg.ntz; ++i) k = max(k, s[i]);
  int32_t e[ALIGN_END_REC];
  align_end_decode(k, lb, lc, e);
  const bool ok = k && e[0] >= 1 && e[0] <= la && e[1] >= 1 && e[1] <= lb && e[2] >= 1 && e[2] <= lc && e[3] >= 0 &&
                  e[3] < NSTATE;
  for (int i = 0; i < ALIGN_END_REC; ++i) endrec[ALIGN_END_REC * t + i] = e[i];
  scores[t] = e[4];
  int32_t *rec = walk + ALIGN_WALK_REC * t;
  rec[0] = e[0], rec[1] = e[1], rec[2] = e[2], rec[3] = e[3], rec[4] = 0, rec[5] = ok ? 0 : 1;
  if (!ok) info[4 * t] = 0;
}

void align_launch_grid_end(const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax, const uint64_t *d_slots,
                           const int64_t *d_slot_off, int32_t *d_scores, int32_t *d_endrec, int32_t *d_walk,
                           int32_t *d_info, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(align_grid_end_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_offsets, n, tymax, tzmax,
                     d_slots, d_slot_off, d_scores, d_endrec, d_walk, d_info);
}

// One launch for n triples: fwd the forward form's launch d over a grid of
// (triple, ndiag indices along the diagonal), otherwise launch d of the
// backward form, triple = workgroup. The tile caps, max_pos and lds as
// align_launch_tiled's; d_tb_off[t] = the word offset of triple t's tile cube,
// d_face_off[t] = the cell offset of its align_grid_face_cells in d_faces.
// end_mode = TSA_END_FACE / TSA_END_ANY: the END forms, with d_slots and
// d_slot_off[t] = the key offset of triple t's nty*ntz slots.
int align_launch_grid(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                      int64_t max_pos, size_t lds, const KParams &kp, bool fwd, int32_t d, int32_t ndiag,
                      const int32_t *d_walk, int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb,
                      const int64_t *d_tb_off, void *d_faces, const int64_t *d_face_off, hipStream_t stream,
                      int32_t end_mode, uint64_t *d_slots, const int64_t *d_slot_off) {
  if (n <= 0) return TSA_OK;
  if (end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY || (end_mode != TSA_END_CORNER && (!d_slots || !d_slot_off)))
    return TSA_EINVAL;
  if (!align_tile_fits(tymax, tzmax) || max_pos < 1 || max_pos > (int64_t)tymax * tzmax || lds > LDS_MAX || !d_tb ||
      !d_tb_off || !d_faces || !d_face_off || !d_walk || d < 0 || (fwd && (ndiag < 1 || ndiag > 65535)))
    return TSA_EINVAL;
  const int k = (int)((max_pos + GRID_NT - 1) / GRID_NT);
  const int nt = (int)(((max_pos + k - 1) / k + 63) / 64 * 64);
  if (fwd && end_mode != TSA_END_CORNER) {  // the forward END form takes the slots where the others take the cubes
    d_tb = (uint32_t *)d_slots;
    d_tb_off = d_slot_off;
  }
  auto launch = [&](auto kfn) {
    return launch_with_lds((const void *)kfn, lds, [&] {
             hipLaunchKernelGGL(kfn, dim3(n, fwd ? ndiag : 1), dim3(nt), lds, stream, d_seqs, d_offsets, kp,
                                (uint32_t)lds, tymax, tzmax, d, d_walk, d_scores, d_final7, d_tb, d_tb_off,
                                (uint4 *)d_faces, d_face_off);
           }) == hipSuccess
               ? TSA_OK
               : TSA_EDEVICE;
  };
  if (fwd && end_mode == TSA_END_FACE) {
    if (k == 1) return launch(align_grid_kernel<1, true, TSA_END_FACE>);
    if (k == 2) return launch(align_grid_kernel<2, true, TSA_END_FACE>);
    return launch(align_grid_kernel<3, true, TSA_END_FACE>);
  }
  if (fwd && end_mode == TSA_END_ANY) {
    if (k == 1) return launch(align_grid_kernel<1, true, TSA_END_ANY>);
    if (k == 2) return launch(align_grid_kernel<2, true, TSA_END_ANY>);
    return launch(align_grid_kernel<3, true, TSA_END_ANY>);
  }
  if (end_mode != TSA_END_CORNER) {  // backward: one form for both modes
    if (k == 1) return launch(align_grid_kernel<1, false, ALIGN_END_PTRS>);
    if (k == 2) return launch(align_grid_kernel<2, false, ALIGN_END_PTRS>);
    return launch(align_grid_kernel<3, false, ALIGN_END_PTRS>);
  }
  if (fwd) {
    if (k == 1) return launch(align_grid_kernel<1, true>);
    if (k == 2) return launch(align_grid_kernel<2, true>);
    return launch(align_grid_kernel<3, true>);
  }
  if (k == 1) return launch(align_grid_kernel<1, false>);
  if (k == 2) return launch(align_grid_kernel<2, false>);
  return launch(align_grid_kernel<3, false>);
}

}  // namespace tsa
