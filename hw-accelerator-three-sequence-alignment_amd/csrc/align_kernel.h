// align_kernel.h -- what the traceback entry points (align_api.hip) launch: the
// resident kernel (align_kernel.hip), the tiled resident kernel
// (align_tiled_kernel.hip), the strip kernel (align_strip_kernel.hip), the grid
// kernels (align_grid_kernel.hip), the batch form of the TB plane sweep and the
// batched walks (plane_kernel.hip); and the helper kernels of the device-resident
// entry points (align_async_kernel.hip). The sizing functions and the plan of a
// triple are __host__ __device__: the host planner and the kernel that builds a
// chunk's metadata on the device read one definition.
#pragma once

#include "tsa_internal.h"

namespace tsa {

// trialign_api.hip's check of a parameter set (1 = usable).
int params_ok(const tsa_params *p);

// The TB plane sweep for a batch: triple t's pointer cube starts at word
// d_tb_off[t] of d_tb, one launch per plane serves all n triples (max_l* over
// the batch). d_tb_off null: tsa_internal.h's form, one triple with exact
// lengths whose cube starts at d_tb.
int plane_launch_batch(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t max_la,
                       int32_t max_lb, int32_t max_lc, const KParams &kp, int32_t *d_scores,
                       int32_t *d_final7, void *d_ws, size_t ws_bytes, hipStream_t stream, uint32_t *d_tb,
                       const int64_t *d_tb_off);

// The walks of n triples in one launch, one walker (thread) per triple:
// triple t's cube at word tb_off[t], its lengths from offs[3t..3t+3], its 7
// final states at final7[7t]; its moves go to moves[offs[3t] ..) in forward
// order and {moves, x0, y0, z0} to info[4t].
__global__ void tb_walk_batch(const uint32_t *tb, const int64_t *tb_off, const int64_t *offs, int32_t n,
                              const int32_t *final7, uint8_t *moves, int32_t *info);

// The resident traceback kernel: one workgroup sweeps a whole cube in one
// launch, its (y,z) planes in LDS. fits: lb*lc positions within the
// workgroup's registers and both planes within LDS (la is not bounded).
// ALIGN_RESIDENT_POS = its 1024 threads x 4 positions, ALIGN_LDS_BYTES = the
// 160 KiB of LDS (pencil_common.h's LDS_MAX); align_kernel.hip asserts both.
constexpr int64_t ALIGN_RESIDENT_POS = 4096;
constexpr size_t ALIGN_LDS_BYTES = 160 * 1024;
__host__ __device__ inline size_t align_cells_bytes(int32_t lb, int32_t lc) {
  return 2 * sizeof(uint4) * (size_t)(lb + 1) * (size_t)(lc + 1);
}
__host__ __device__ inline bool align_resident_fits(int32_t la, int32_t lb, int32_t lc) {
  (void)la;  // A is staged when it fits and read from global memory when not
  return (int64_t)lb * lc <= ALIGN_RESIDENT_POS && align_cells_bytes(lb, lc) + lb + lc <= ALIGN_LDS_BYTES;
}
// Dynamic LDS a (la,lb,lc) triple asks for (A staged when there is room).
__host__ __device__ inline size_t align_resident_lds(int32_t la, int32_t lb, int32_t lc) {
  size_t need = align_cells_bytes(lb, lc) + (size_t)lb + lc;
  if (need + (size_t)la <= ALIGN_LDS_BYTES) need += la;
  need = (need + 15) & ~(size_t)15;
  return need < ALIGN_LDS_BYTES ? need : ALIGN_LDS_BYTES;
}
// Bytes of the pointer cube of one (la,lb,lc) triple: tsa_internal.h's
// tb_cube_bytes (plane_kernel.hip, host only) returns this.
__host__ __device__ inline size_t align_cube_bytes(int32_t la, int32_t lb, int32_t lc) {
  return (size_t)lb * (size_t)(la + lc - 1) * (size_t)lc * sizeof(uint32_t);
}
// One launch for n triples that all fit, through launch_with_lds (so
// tsa_kernel_launch_count counts it): max_pos = the largest lb*lc and lds =
// the largest align_resident_lds of the batch.
// end_mode = TSA_END_FACE / TSA_END_ANY (tsa_align_batch_ends): the kernel
// searches the end cell as it sweeps and writes the triple's end record
// (below) to d_endrec[5t] and its MAX7 to d_scores[t]; d_final7 is not written.
int align_launch_resident(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int64_t max_pos, size_t lds,
                          const KParams &kp, int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb,
                          const int64_t *d_tb_off, hipStream_t stream, int32_t end_mode = TSA_END_CORNER,
                          int32_t *d_endrec = nullptr);

// The end record of a triple under tsa_align_batch_ends, int32 words
// {x1, y1, z1, state, score}: the cell and the state the path ends in and that
// cell's MAX7. The kernels find it through a 64-bit key per cell (align_step.h)
// whose position field holds the cell's number in (x,y,z) order, below la*lb*lc.
constexpr int ALIGN_END_REC = 5;
// AlignPos::step's END of a sweep that follows the search (the backward END
// form of the grid kernels): neither an end key nor the corner's score.
constexpr int ALIGN_END_PTRS = -1;
constexpr int ALIGN_END_POS_BITS = 45;
constexpr uint64_t ALIGN_END_POS_MASK = (1ull << ALIGN_END_POS_BITS) - 1;
// Every cube whose pointers fit device memory passes: it has more than
// la*lb*lc words of 4 bytes.
__host__ __device__ inline bool align_end_key_fits(int32_t la, int32_t lb, int32_t lc) {
  const uint64_t lim = 1ull << ALIGN_END_POS_BITS, plane = (uint64_t)lb * (uint64_t)lc;  // below 2^62
  return plane <= lim && (uint64_t)la <= lim / plane;
}
// The walks of n triples from their end records, one walker (thread) per
// triple, otherwise as tb_walk_batch: the cube is indexed with the full lengths.
__global__ void tb_walk_ends(const uint32_t *tb, const int64_t *tb_off, const int64_t *offs, int32_t n,
                             const int32_t *endrec, uint8_t *moves, int32_t *info);

// The tiled resident kernel (align_tiled_kernel.hip): one workgroup sweeps a
// cube whose (y,z) plane does not fit it, tile by tile, the tiles chained
// through face buffers in global memory. Balanced tiles under the caps
// tymax x tzmax (align_tile_fits): nty = ceil(lb/tymax) tiles of
// TY = ceil(lb/nty) rows (the last one shorter, never empty), likewise along z.
struct AlignTileGeom {
  int32_t TY, TZ, nty, ntz;
};
__host__ __device__ inline AlignTileGeom align_tile_geom(int32_t lb, int32_t lc, int32_t tymax, int32_t tzmax) {
  AlignTileGeom g;
  g.nty = (lb + tymax - 1) / tymax;
  g.ntz = (lc + tzmax - 1) / tzmax;
  g.TY = (lb + g.nty - 1) / g.nty;
  g.TZ = (lc + g.ntz - 1) / g.ntz;
  return g;
}
// A tile the tiled kernel can sweep: within the resident capacity
// (align_resident_fits) and within 3 positions per thread of a 1024-thread
// workgroup -- the fourth position the resident kernel has would spill here.
bool align_tile_fits(int32_t ty, int32_t tz);
// The default tile caps: 3072 positions, a row of B symbols as deep as the
// resident kernel's.
constexpr int32_t ALIGN_TILE_Y = 64, ALIGN_TILE_Z = 48;
// 16-byte cells of a triple's face workspace: two y faces [la][lc+1] and two
// z faces [la][TY].
__host__ __device__ inline size_t align_tiled_face_cells(int32_t la, int32_t lb, int32_t lc, int32_t tymax,
                                                         int32_t tzmax) {
  const AlignTileGeom g = align_tile_geom(lb, lc, tymax, tzmax);
  return 2 * (size_t)la * ((size_t)lc + 1) + 2 * (size_t)la * (size_t)g.TY;
}
// One launch for n triples through launch_with_lds: max_pos = the largest
// TY*TZ and lds = the largest align_resident_lds(la, TY, TZ) of the batch;
// d_face_off[t] = the cell offset of triple t's face workspace in d_faces.
int align_launch_tiled(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                       int64_t max_pos, size_t lds, const KParams &kp, int32_t *d_scores, int32_t *d_final7,
                       uint32_t *d_tb, const int64_t *d_tb_off, void *d_faces, const int64_t *d_face_off,
                       hipStream_t stream, int32_t end_mode = TSA_END_CORNER, int32_t *d_endrec = nullptr);

// The strip kernel (align_strip_kernel.hip): a strip is one tile row of the
// tiled kernel, TY rows of y with all of z and x. A forward launch keeps the y
// face of every strip but the last; strip launch j then sweeps strip
// nty-1-j of every triple again, with pointers, into a cube of one strip, and
// tb_walk_strip follows them before launch j+1 overwrites it.
// Bytes of a triple's strip cube, TY*(la+lc-1)*lc words.
__host__ __device__ inline size_t align_strip_cube_bytes(int32_t la, int32_t lb, int32_t lc, int32_t tymax,
                                                         int32_t tzmax) {
  const AlignTileGeom g = align_tile_geom(lb, lc, tymax, tzmax);
  return sizeof(uint32_t) * (size_t)g.TY * (size_t)(la + lc - 1) * (size_t)lc;
}
// 16-byte cells of its face workspace: nty-1 kept y faces [la][lc+1] and two
// z faces [la][TY].
__host__ __device__ inline size_t align_strip_face_cells(int32_t la, int32_t lb, int32_t lc, int32_t tymax,
                                                         int32_t tzmax) {
  const AlignTileGeom g = align_tile_geom(lb, lc, tymax, tzmax);
  return (size_t)(g.nty - 1) * (size_t)la * ((size_t)lc + 1) + 2 * (size_t)la * (size_t)g.TY;
}
// The walker record of a triple, int32 words {x, y, z, T, n, done}: where the
// walk stands, the state it is in, the moves it has made and whether the path
// has reached a zero face.
constexpr int ALIGN_WALK_REC = 6;
// One launch for n triples through launch_with_lds: j < 0 the forward form
// (strips 0 .. nty-2, no pointers), j >= 0 strip launch j, which skips a triple
// with fewer than j+1 strips or whose record in d_walk is done. max_pos, lds
// and d_face_off as align_launch_tiled's, over align_strip_face_cells;
// d_tb_off[t] = the word offset of triple t's strip cube.
int align_launch_strip(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                       int64_t max_pos, size_t lds, const KParams &kp, int32_t j, const int32_t *d_walk,
                       int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb, const int64_t *d_tb_off, void *d_faces,
                       const int64_t *d_face_off, hipStream_t stream);
// The walk after strip launch j, one walker (thread) per triple: it follows
// the pointers of strip s = nty-1-j from where its record in walk stands (from
// (la,lb,lc) and final7 when j = 0) while the cell lies in the strip, y > s*TY,
// appending to moves[offs[3t] ..) from the end backwards. A predecessor on a
// zero face ends the path: done is set, {moves, x0, y0, z0} go to info[4t] and
// the walker reverses its slice into forward order. A predecessor in the strip
// below saves the record for launch j+1.
__global__ void tb_walk_strip(const uint32_t *tb, const int64_t *tb_off, const int64_t *offs, int32_t n,
                              int32_t tymax, int32_t tzmax, int32_t j, const int32_t *final7, int32_t *walk,
                              uint8_t *moves, int32_t *info);

// The grid kernels (align_grid_kernel.hip): the tiled kernel's tiles, every one
// checkpointed. Forward launch d sweeps the tiles with ty + tz = d of every
// triple, one workgroup each, and keeps the y face of every tile row but the
// last and the z face of every tile column but the last; backward launch j then
// sweeps again, with pointers into a cube of one tile, the tile the triple's
// walker stands in, up to the walker's x, and tb_walk_grid follows them before
// launch j+1 overwrites it.
// Bytes of a triple's tile cube, TY*(la+TZ-1)*TZ words.
__host__ __device__ inline size_t align_grid_cube_bytes(int32_t la, int32_t lb, int32_t lc, int32_t tymax,
                                                        int32_t tzmax) {
  const AlignTileGeom g = align_tile_geom(lb, lc, tymax, tzmax);
  return sizeof(uint32_t) * (size_t)g.TY * (size_t)(la + g.TZ - 1) * (size_t)g.TZ;
}
// 16-byte cells of its kept faces: nty-1 y faces [la][lc+1] and ntz-1 z faces
// [la][lb]. A grid triple's need against the budget is the sum of both:
//   4*TY*(la+TZ-1)*TZ + 16*((nty-1)*la*(lc+1) + (ntz-1)*la*lb)  bytes.
__host__ __device__ inline size_t align_grid_face_cells(int32_t la, int32_t lb, int32_t lc, int32_t tymax,
                                                        int32_t tzmax) {
  const AlignTileGeom g = align_tile_geom(lb, lc, tymax, tzmax);
  return (size_t)(g.nty - 1) * (size_t)la * ((size_t)lc + 1) + (size_t)(g.ntz - 1) * (size_t)la * (size_t)lb;
}
// One launch through launch_with_lds. fwd: launch d of the forward form over
// (n triples) x (ndiag indices along the diagonal, the most tiles any triple
// has on one); a workgroup without a tile on diagonal d, or with the last tile,
// leaves at once. Otherwise launch d of the backward form, one workgroup per
// triple, which skips a triple whose record in d_walk is done (d = 0 reads no
// record: the tile of (lb,lc), all of x). max_pos, lds and d_face_off as
// align_launch_tiled's, over align_grid_face_cells; d_tb_off[t] = the word
// offset of triple t's tile cube.
// end_mode = TSA_END_FACE / TSA_END_ANY (tsa_align_batch_grid_ends): the END
// forms. Forward launch d = 0 .. nty+ntz-2 sweeps the last tile too, and every
// tile stores the largest end key of its cells into its own slot,
// d_slots[d_slot_off[t] + ty*ntz + tz]; align_launch_grid_end then makes the
// records; backward launch d = 0 reads the triple's record like every later
// one and no backward launch writes d_scores or d_final7.
int align_launch_grid(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax,
                      int64_t max_pos, size_t lds, const KParams &kp, bool fwd, int32_t d, int32_t ndiag,
                      const int32_t *d_walk, int32_t *d_scores, int32_t *d_final7, uint32_t *d_tb,
                      const int64_t *d_tb_off, void *d_faces, const int64_t *d_face_off, hipStream_t stream,
                      int32_t end_mode = TSA_END_CORNER, uint64_t *d_slots = nullptr,
                      const int64_t *d_slot_off = nullptr);
// After the last forward END launch, one thread per triple (not a counted
// launch): the max over the triple's nty*ntz slots, decoded into d_scores[t],
// the end record d_endrec[5t ..] and the walker record d_walk[6t ..] =
// {x1, y1, z1, state, 0, 0}. A key that names no cell of the cube marks the
// record done and sets d_info[4t] = 0 moves (TSA_EINTERNAL on the host).
void align_launch_grid_end(const int64_t *d_offsets, int32_t n, int32_t tymax, int32_t tzmax, const uint64_t *d_slots,
                           const int64_t *d_slot_off, int32_t *d_scores, int32_t *d_endrec, int32_t *d_walk,
                           int32_t *d_info, hipStream_t stream);
// The walk after backward launch j, one walker (thread) per triple: it follows
// the pointers of the tile its record stands in (from (la,lb,lc) and final7
// when j = 0) while the cell lies in that tile, appending to moves[offs[3t] ..)
// from the end backwards. A predecessor on a zero face ends the path as in
// tb_walk_strip; one in another tile -- through a y seam, a z seam or the
// corner -- saves the record for launch j+1.
__global__ void tb_walk_grid(const uint32_t *tb, const int64_t *tb_off, const int64_t *offs, int32_t n,
                             int32_t tymax, int32_t tzmax, int32_t j, const int32_t *final7, int32_t *walk,
                             uint8_t *moves, int32_t *info);

// ---- the plan of a triple (align_api.hip plans with it on the host,
// align_meta_kernel on the device) ------------------------------------------
// The plan mode: the override align_mode, or what the entry point plans when
// it is not set (auto, strip under tsa_align_batch_lowmem, grid under
// tsa_align_batch_grid, the path argument of tsa_align_batch_async).
enum AlignMode {
  ALIGN_MODE_AUTO, ALIGN_MODE_RESIDENT, ALIGN_MODE_PLANE, ALIGN_MODE_TILED, ALIGN_MODE_STRIP, ALIGN_MODE_GRID
};
// Passed to the meta kernel by value.
struct AlignPlan {
  int32_t mode = ALIGN_MODE_AUTO;
  int32_t mode_set = 0;  // align_mode is set
  int32_t capped = 0;    // align_tile is set
  int32_t tymax = ALIGN_TILE_Y, tzmax = ALIGN_TILE_Z;
  int32_t end_mode = 0;  // TSA_END_FACE / TSA_END_ANY: every over-capacity triple is tiled, or grid under mode = grid
};
// Over capacity: the triple does not go to the resident kernel as a whole.
// With align_tile set under align_mode = tiled, strip or grid that is any triple
// larger than the tile (tests put tiny cubes through many tiles that way).
__host__ __device__ inline bool align_over(const AlignPlan &pl, int32_t la, int32_t lb, int32_t lc) {
  if ((pl.mode == ALIGN_MODE_TILED || pl.mode == ALIGN_MODE_STRIP || pl.mode == ALIGN_MODE_GRID) && pl.capped)
    return lb > pl.tymax || lc > pl.tzmax;
  return !align_resident_fits(la, lb, lc);
}
// What a triple asks of the device buffers: whether it is over capacity (under
// align_mode = plane every triple is), the bytes of its pointer cube -- of its
// strip cube on the strip path, its tile cube on the grid path -- and the
// 16-byte cells of its face workspace if it is tiled, strips or grid.
struct AlignNeed {
  bool over;
  size_t cube, face;
};
__host__ __device__ inline AlignNeed align_need(const AlignPlan &pl, int32_t la, int32_t lb, int32_t lc) {
  AlignNeed t;
  t.over = pl.mode == ALIGN_MODE_PLANE || align_over(pl, la, lb, lc);
  const bool strip = t.over && pl.mode == ALIGN_MODE_STRIP, grid = t.over && pl.mode == ALIGN_MODE_GRID;
  t.cube = strip  ? align_strip_cube_bytes(la, lb, lc, pl.tymax, pl.tzmax)
           : grid ? align_grid_cube_bytes(la, lb, lc, pl.tymax, pl.tzmax)
                  : align_cube_bytes(la, lb, lc);
  t.face = strip    ? align_strip_face_cells(la, lb, lc, pl.tymax, pl.tzmax)
           : grid   ? align_grid_face_cells(la, lb, lc, pl.tymax, pl.tzmax)
           : t.over ? align_tiled_face_cells(la, lb, lc, pl.tymax, pl.tzmax)
                    : 0;
  return t;
}

// ---- the helper kernels of tsa_align_batch_async, tsa_align_batch_ends_async
// and tsa_align_rows_async (align_async_kernel.hip). None is counted by tsa_kernel_launch_count. ------
// The buffers of one chunk of m triples, caller's triples [i0, i0 + m), in
// launch order: the resident triples first, then the over-capacity ones, each
// group in the caller's order. What align_run builds on the host for the
// synchronous entry points, align_launch_meta builds on the device.
struct AlignChunkBufs {
  int64_t *off;       // 3m+1 offsets of the packed sequences, from 0
  int64_t *tb_off;    // m word offsets of the cubes, an exclusive scan
  int64_t *face_off;  // m cell offsets of the face workspaces, an exclusive scan
  int32_t *order;     // m: the caller's index of launch slot j
  int32_t *scores;    // m
  int32_t *final7;    // 7m
  int32_t *info;      // 4m {moves, x0, y0, z0}, zeroed by the meta kernel
  uint8_t *seqs;      // the packed sequences
  uint8_t *moves;     // the moves, laid out as seqs
  // tsa_align_batch_ends_async alone, null elsewhere:
  int64_t *slot_off;  // m key offsets of the grid triples' slots, an exclusive scan (grid path with a free end)
  int32_t *endrec;    // 5m end records (TSA_END_FACE, TSA_END_ANY); they lie on final7, as in align_run
};
// One workgroup: reads d_offsets[3*i0 .. 3*(i0+m)] and fills off, tb_off,
// face_off and order of the chunk under plan pl (align_need of every triple),
// and zeroes info. With b.slot_off set (the grid path with a free end) it fills
// that as well: nty*ntz keys per over-capacity triple, 0 for a resident one.
void align_launch_meta(const int64_t *d_offsets, int32_t i0, int32_t m, const AlignPlan &pl, const AlignChunkBufs &b,
                       hipStream_t stream);
// One workgroup per triple: copies its la+lb+lc symbols from the caller's
// d_seqs to its packed place b.seqs + b.off[3j].
void align_launch_pack(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t m, const AlignChunkBufs &b,
                       hipStream_t stream);
// One workgroup per triple: score, n_moves (0 unless 1 <= moves <= la+lb+lc)
// and start to the caller's index, and exactly n_moves bytes of moves to the
// caller's slot d_moves + d_offsets[3i] - d_offsets[0]. With d_ends set
// (tsa_align_batch_ends_async) the END form: also d_ends[3i..3i+2], the cell of
// the triple's end record b.endrec[5j ..], or its lengths when b.endrec is null
// (TSA_END_CORNER).
void align_launch_finish(const int64_t *d_offsets, int32_t m, const AlignChunkBufs &b, int32_t *d_scores,
                         uint8_t *d_moves, int32_t *d_n_moves, int32_t *d_starts, hipStream_t stream,
                         int32_t *d_ends = nullptr);
// The gapped rows of n alignments, one wave per triple (tsa_align_rows_async).
void align_launch_rows(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, const uint8_t *d_moves,
                       const int32_t *d_n_moves, const int32_t *d_starts, uint8_t *d_rows, hipStream_t stream);

}  // namespace tsa
