// align_api.hip -- the traceback entry points of include/trialign.h:
// tsa_align_batch, tsa_align_batch_lowmem, tsa_align_batch_grid, tsa_align_batch_ends
// (tsa_align_batch with a free end: the resident and the tiled kernel search
// the end cell as they sweep, tb_walk_ends walks from it), tsa_align_batch_grid_ends
// (the same search by the grid kernels, a key per tile), tsa_align_gpu
// (one triple, always the plane sweep), tsa_describe_align_plan and the
// device-resident tsa_align_workspace_size, tsa_align_batch_async,
// tsa_align_ends_workspace_size, tsa_align_batch_ends_async (the free end on
// that path) and tsa_align_rows_async, which plan with the same planner against a caller's
// workspace and queue the same launches (helper kernels: align_async_kernel.hip). Host code
// only: which path a triple takes, the chunks of pointer cubes, the device buffers and the
// launches of the resident kernel (align_kernel.hip), the tiled resident kernel
// (align_tiled_kernel.hip), the strip kernel (align_strip_kernel.hip), the grid
// kernels (align_grid_kernel.hip), the batched plane sweep and the batched
// walks (plane_kernel.hip).
//
// Traceback is an extension: the reference's alignment-output ports are
// commented out (src/TriAlign_tb.sv:239-260).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "align_kernel.h"

using namespace tsa;

namespace {
// Device buffers and the stream of one call, released on every exit path.
struct AlignBufs {
  std::vector<void *> ptrs;
  hipStream_t s = nullptr;
  template <class T>
  bool alloc(T **p, size_t bytes) {
    void *v = nullptr;
    if (hipMalloc(&v, std::max<size_t>(bytes, 16)) != hipSuccess) return false;
    ptrs.push_back(v);
    *p = (T *)v;
    return true;
  }
  ~AlignBufs() {
    for (void *v : ptrs) (void)hipFree(v);
    if (s) (void)hipStreamDestroy(s);
  }
};

// Which path a triple takes. One that fits a workgroup is swept by the resident
// kernel (one launch per chunk): on the MI355X it was the faster path on every
// recorded shape it holds (profiles/align_batch.jsonl). One that does not fit
// is swept tile by tile by the tiled resident kernel (one more launch per
// chunk) or by the batched plane sweep. The tiled kernel runs one workgroup
// per triple, so it needs a group large enough to fill the device: without an
// override, the over-capacity triples of a chunk are tiled when there are at
// least kAlignTiledMinGroup of them (profiles/align_tiled.jsonl)
// and take the plane sweep otherwise. Under align_mode = strip (what
// tsa_align_batch_lowmem plans by default) they take the strip path instead,
// which keeps the pointers of one tile row of a cube at a time: never chosen
// without being asked for, since it sweeps most cells twice. Under align_mode =
// grid (what tsa_align_batch_grid plans by default) they take the grid path,
// which keeps the faces of every tile, sweeps the tiles of a diagonal of the
// tile grid as workgroups of their own and sweeps again, with the pointers of
// one tile, only the tiles on the path: opt-in as well.
enum AlignPath { ALIGN_RESIDENT, ALIGN_TILED, ALIGN_PLANE, ALIGN_STRIP, ALIGN_GRID };
// 256 = the smallest measured group from which the tiled kernel's median beat the
// plane sweep's beyond the spread of the passes on every shape (128^3 and 256^3;
// at 64 triples the plane sweep still wins both): one workgroup per CU.
constexpr int32_t kAlignTiledMinGroup = 256;

// The overrides align_mode and align_tile; TSA_EINVAL for a value outside
// include/trialign.h's.
int align_plan_read(AlignPlan *pl) {
  char v[64];
  *pl = AlignPlan();
  if (override_str("align_mode", v, sizeof v)) {
    if (!strcmp(v, "resident")) pl->mode = ALIGN_MODE_RESIDENT;
    else if (!strcmp(v, "plane")) pl->mode = ALIGN_MODE_PLANE;
    else if (!strcmp(v, "tiled")) pl->mode = ALIGN_MODE_TILED;
    else if (!strcmp(v, "strip")) pl->mode = ALIGN_MODE_STRIP;
    else if (!strcmp(v, "grid")) pl->mode = ALIGN_MODE_GRID;
    else return TSA_EINVAL;
    pl->mode_set = true;
  }
  if (override_str("align_tile", v, sizeof v)) {  // "TYxTZ", decimal digits only
    long e[2] = {0, 0};
    const char *s = v;
    for (int k = 0; k < 2; ++k) {
      if (*s < '0' || *s > '9') return TSA_EINVAL;
      for (; *s >= '0' && *s <= '9'; ++s)
        if ((e[k] = e[k] * 10 + (*s - '0')) > 65536) return TSA_EINVAL;
      if (*s != (k ? '\0' : 'x')) return TSA_EINVAL;
      ++s;
    }
    if (!align_tile_fits((int32_t)e[0], (int32_t)e[1])) return TSA_EINVAL;
    pl->capped = true;
    pl->tymax = (int32_t)e[0], pl->tzmax = (int32_t)e[1];
  }
  return TSA_OK;
}

// The path of the over-capacity triples of a group that holds n_over of them.
AlignPath align_over_path(const AlignPlan &pl, int32_t n_over) {
  // tsa_align_batch_ends: tiled, whatever their number; tsa_align_batch_grid_ends: grid
  if (pl.end_mode != TSA_END_CORNER) return pl.mode == ALIGN_MODE_GRID ? ALIGN_GRID : ALIGN_TILED;
  if (pl.mode == ALIGN_MODE_TILED) return ALIGN_TILED;
  if (pl.mode == ALIGN_MODE_STRIP) return ALIGN_STRIP;
  if (pl.mode == ALIGN_MODE_GRID) return ALIGN_GRID;
  if (pl.mode == ALIGN_MODE_AUTO && n_over >= kAlignTiledMinGroup) return ALIGN_TILED;
  return ALIGN_PLANE;
}

AlignPath align_path(const AlignPlan &pl, int32_t la, int32_t lb, int32_t lc, int32_t n_over) {
  if (pl.mode == ALIGN_MODE_PLANE) return ALIGN_PLANE;
  if (!align_over(pl, la, lb, lc)) return ALIGN_RESIDENT;
  return align_over_path(pl, n_over);
}

// What the call plans for one triple, computed once: the sizing of the
// buffers, the chunks and the launches all read these numbers.
struct AlignTriple {
  int32_t la, lb, lc;
  bool over;     // not the resident kernel's: tiled or plane, as its chunk decides, or strip, or grid
  size_t cube;   // bytes of its pointer cube; of its strip cube on the strip path, its tile cube on the grid path
  size_t face;   // 16-byte cells of its face workspace if the chunk is tiled, strips or grid
  size_t need;   // what it takes of the budget: the cube; with the faces on the strip and grid paths (O(N^3/TY))
  int32_t nty;   // its strips on the strip path
  int32_t ntz;   // with nty its tile grid on the grid path
  int64_t pos;   // positions of its workgroup: lb*lc, or TY*TZ of an over-capacity triple's tiles
  size_t lds;    // align_resident_lds of that plane or tile
};
// Consecutive triples [i0, i1) whose needs fit the budget together, as a batch
// of its own: what its launches and the buffers need.
struct AlignChunk {
  int32_t i0, i1, n_over = 0;
  bool tiled = false, strip = false, grid = false;  // the path of the n_over over-capacity triples
  int32_t max_nty = 0;                    // the strip launches: the most strips of a triple
  int32_t max_diag = 0, max_len = 0;      // the grid launches: the most diagonals (nty+ntz-1), the longest diagonal
  size_t slots = 0;                       // the end keys of its grid triples, one per tile (tsa_align_batch_grid_ends)
  size_t need = 0, cube = 0, seq = 0;     // bytes against the budget, of the cubes and of the sequences
  int64_t max_pos = 1, tile_pos = 1;      // the resident and the tiled launch
  size_t lds = 0, tile_lds = 0, face = 0; // face: bytes
  int32_t mla = 1, mlb = 1, mlc = 1;      // the plane sweep
  size_t ws = 0;
};

// The plan of n validated triples under pl, from (a host copy of) their
// offsets. tiled_faces: a tiled triple's face workspace counts against the
// budget as well (tsa_align_batch_async, whose faces and cubes share one
// workspace; the synchronous entry points allocate the tiled faces apart).
std::vector<AlignTriple> align_plan_triples(const int64_t *offsets, int32_t n, const AlignPlan &pl, bool tiled_faces) {
  std::vector<AlignTriple> T((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    const int64_t *o = offsets + 3 * (int64_t)i;
    AlignTriple &t = T[i];
    t.la = (int32_t)(o[1] - o[0]), t.lb = (int32_t)(o[2] - o[1]), t.lc = (int32_t)(o[3] - o[2]);
    const AlignNeed nd = align_need(pl, t.la, t.lb, t.lc);
    t.over = nd.over, t.cube = nd.cube, t.face = nd.face;
    const bool kept = t.over && (pl.mode == ALIGN_MODE_STRIP || pl.mode == ALIGN_MODE_GRID || tiled_faces);
    const AlignTileGeom g = t.over ? align_tile_geom(t.lb, t.lc, pl.tymax, pl.tzmax) : AlignTileGeom{t.lb, t.lc, 1, 1};
    t.need = t.cube + (kept ? sizeof(uint4) * t.face : 0);
    t.nty = g.nty, t.ntz = g.ntz;
    t.pos = (int64_t)g.TY * g.TZ;
    t.lds = align_resident_lds(t.la, g.TY, g.TZ);
  }
  return T;
}

// The chunks of the planned triples T: consecutive triples whose needs fit
// `budget` together, at most 65535. TSA_ENOMEM when one triple's own need
// exceeds the budget, as a failed allocation.
int align_plan_chunks(const std::vector<AlignTriple> &T, const AlignPlan &pl, size_t budget,
                      std::vector<AlignChunk> *chunks) {
  const int32_t n = (int32_t)T.size();
  for (int32_t i = 0; i < n;) {
    AlignChunk c;  // the over-capacity triples' needs for both of their paths, until their number decides
    int32_t j = i;
    for (; j < n && j - i < 65535; ++j) {
      const AlignTriple &t = T[j];
      if (t.need > budget) return TSA_ENOMEM;
      if (t.need > budget - c.need) break;
      c.need += t.need;
      c.cube += t.cube;
      c.seq += (size_t)t.la + t.lb + t.lc;
      if (!t.over) {
        c.max_pos = std::max(c.max_pos, t.pos), c.lds = std::max(c.lds, t.lds);
        continue;
      }
      ++c.n_over;
      c.tile_pos = std::max(c.tile_pos, t.pos), c.tile_lds = std::max(c.tile_lds, t.lds);
      c.face += sizeof(uint4) * t.face;
      c.max_nty = std::max(c.max_nty, t.nty);
      c.max_diag = std::max(c.max_diag, t.nty + t.ntz - 1), c.max_len = std::max(c.max_len, std::min(t.nty, t.ntz));
      c.slots += (size_t)t.nty * t.ntz;
      c.mla = std::max(c.mla, t.la), c.mlb = std::max(c.mlb, t.lb), c.mlc = std::max(c.mlc, t.lc);
    }
    c.i0 = i, c.i1 = j;
    c.tiled = c.n_over && align_over_path(pl, c.n_over) == ALIGN_TILED;
    c.strip = c.n_over && align_over_path(pl, c.n_over) == ALIGN_STRIP;
    c.grid = c.n_over && align_over_path(pl, c.n_over) == ALIGN_GRID;
    if (!c.tiled && !c.strip && !c.grid)
      c.face = 0, c.ws = c.n_over ? plane_workspace_bytes(c.n_over, c.mla, c.mlb, c.mlc) : 0;
    chunks->push_back(c);
    i = j;
  }
  return TSA_OK;
}

// The device buffers of one chunk as its launches see them: the sequences
// packed in launch order -- the resident triples first, then the over-capacity
// ones (tiled, plane, strip or grid, one path for all of a chunk), so each path
// sees a contiguous sub-batch -- with their offsets, cube word offsets and face
// cell offsets, the results (m scores, 7m final states, 4m walk infos) and the
// moves, laid out as the sequences.
struct AlignDev {
  const uint8_t *seqs;
  const int64_t *off, *tboff, *faceoff;
  int32_t *scores, *final7, *info;
  uint8_t *moves;
  uint32_t *tb;
  void *faces, *ws;
  int32_t *walk;  // the walker records of a chunk's strip or grid triples
  // The end records of the chunk under tsa_align_batch_ends (TSA_END_FACE,
  // TSA_END_ANY), ALIGN_END_REC words a triple; they lie on final7, which the
  // kernels of those modes do not write.
  int32_t *endrec;
  // The end keys of the chunk's grid triples under tsa_align_batch_grid_ends,
  // one slot per tile, and the key offset of every triple's slots (entry mr on
  // is the first grid triple's, as tboff's).
  uint64_t *slots;
  const int64_t *slotoff;
};

// Queues the sweeps and walks of chunk c on stream s.
int align_queue_chunk(const AlignChunk &c, const AlignPlan &pl, const KParams &kp, const AlignDev &d, hipStream_t s) {
  const int32_t m = c.i1 - c.i0, mr = m - c.n_over;
  int rc = TSA_OK;
  if (mr && (rc = align_launch_resident(d.seqs, d.off, mr, c.max_pos, c.lds, kp, d.scores, d.final7, d.tb, d.tboff, s,
                                        pl.end_mode, d.endrec)))
    return rc;
  if (c.tiled)
    rc = align_launch_tiled(d.seqs, d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, c.tile_pos, c.tile_lds, kp,
                            d.scores + mr, d.final7 + (size_t)NSTATE * mr, d.tb, d.tboff + mr, d.faces,
                            d.faceoff + mr, s, pl.end_mode,
                            pl.end_mode != TSA_END_CORNER ? d.endrec + (size_t)ALIGN_END_REC * mr : nullptr);
  else if (c.n_over && !c.strip && !c.grid)
    rc = plane_launch_batch(d.seqs, d.off + 3 * (size_t)mr, c.n_over, c.mla, c.mlb, c.mlc, kp, d.scores + mr,
                            d.final7 + (size_t)NSTATE * mr, d.ws, c.ws, s, d.tb, d.tboff + mr);
  if (rc) return rc;
  // the strip and grid triples are walked segment by segment below; every other one has its whole cube
  const int32_t mw = c.strip || c.grid ? mr : m;
  if (mw && pl.end_mode != TSA_END_CORNER)
    hipLaunchKernelGGL(tb_walk_ends, dim3((mw + 63) / 64), dim3(64), 0, s, d.tb, d.tboff, d.off, mw, d.endrec,
                       d.moves, d.info);
  else if (mw)
    hipLaunchKernelGGL(tb_walk_batch, dim3((mw + 63) / 64), dim3(64), 0, s, d.tb, d.tboff, d.off, mw, d.final7,
                       d.moves, d.info);
  if (c.strip) {
    // forward: the y faces of every strip but the last; then the strips, last
    // to first, each followed by the walk of its pointers. j < 0: the forward form.
    for (int32_t j = c.max_nty >= 2 ? -1 : 0; j < c.max_nty; ++j) {
      if ((rc = align_launch_strip(d.seqs, d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, c.tile_pos,
                                   c.tile_lds, kp, j, d.walk, d.scores + mr, d.final7 + (size_t)NSTATE * mr, d.tb,
                                   d.tboff + mr, d.faces, d.faceoff + mr, s)))
        return rc;
      if (j >= 0)
        hipLaunchKernelGGL(tb_walk_strip, dim3((c.n_over + 63) / 64), dim3(64), 0, s, d.tb, d.tboff + mr,
                           d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, j, d.final7 + (size_t)NSTATE * mr,
                           d.walk, d.moves, d.info + 4 * (size_t)mr);
    }
  }
  if (c.grid) {
    // forward: diagonal by diagonal, every tile but the last of each triple;
    // then the tile each walker stands in, followed by the walk of its pointers,
    // as often as the longest path can change tiles. With a free end the
    // forward form sweeps the last tile as well, one diagonal more, and the end
    // records follow it: the walks then start from their records (j + 1), and
    // the host, which does not know the end tiles, still queues the worst case
    // of backward launches.
    const bool ends = pl.end_mode != TSA_END_CORNER;
    const int32_t nfwd = ends ? c.max_diag : c.max_diag - 1;
    for (int32_t j = 0; j < nfwd + c.max_diag; ++j) {
      const bool fwd = j < nfwd;
      const int32_t dg = fwd ? j : j - nfwd;
      if ((rc = align_launch_grid(d.seqs, d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, c.tile_pos,
                                  c.tile_lds, kp, fwd, dg, c.max_len, d.walk, d.scores + mr,
                                  d.final7 + (size_t)NSTATE * mr, d.tb, d.tboff + mr, d.faces, d.faceoff + mr, s,
                                  pl.end_mode, d.slots, ends ? d.slotoff + mr : nullptr)))
        return rc;
      if (ends && j == nfwd - 1)
        align_launch_grid_end(d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, d.slots, d.slotoff + mr,
                              d.scores + mr, d.endrec + (size_t)ALIGN_END_REC * mr, d.walk, d.info + 4 * (size_t)mr, s);
      if (!fwd)
        hipLaunchKernelGGL(tb_walk_grid, dim3((c.n_over + 63) / 64), dim3(64), 0, s, d.tb, d.tboff + mr,
                           d.off + 3 * (size_t)mr, c.n_over, pl.tymax, pl.tzmax, ends ? dg + 1 : dg,
                           d.final7 + (size_t)NSTATE * mr, d.walk, d.moves, d.info + 4 * (size_t)mr);
    }
  }
  return TSA_OK;
}

// The traceback of n validated triples on the current device: plan pl, chunks
// of at most `budget` bytes of pointer cubes. Outputs as tsa_align_batch's;
// ends (tsa_align_batch_ends, null otherwise) gets the end cell of every triple.
int align_run(const uint8_t *seqs, const int64_t *offsets, int32_t n, const KParams &kp, const AlignPlan &pl,
              size_t budget, int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t *ends) {
  const std::vector<AlignTriple> T = align_plan_triples(offsets, n, pl, false);
  std::vector<AlignChunk> chunks;
  int rc = align_plan_chunks(T, pl, budget, &chunks);
  if (rc) return rc;
  // the end keys of a chunk's grid triples: beside the walker records, outside the budget like them
  const bool keyed = pl.end_mode != TSA_END_CORNER && pl.mode == ALIGN_MODE_GRID;
  size_t max_cube = 0, max_seq = 0, max_ws = 0, max_face = 0, max_slots = 0;
  int32_t max_n = 0;
  for (const AlignChunk &c : chunks) {
    max_cube = std::max(max_cube, c.cube), max_seq = std::max(max_seq, c.seq);
    max_ws = std::max(max_ws, c.ws), max_face = std::max(max_face, c.face);
    if (keyed && c.grid) max_slots = std::max(max_slots, c.slots);
    max_n = std::max(max_n, c.i1 - c.i0);
  }
  // device buffers, once per call, sized for the largest chunk
  AlignBufs B;
  uint8_t *d_seqs = nullptr, *d_moves = nullptr;
  int64_t *d_meta = nullptr;  // [0, 3m] offsets, then m cube word offsets, m face cell offsets, m slot offsets
  int32_t *d_res = nullptr;   // m scores, 7m final states, 4m walk infos
  uint32_t *d_tb = nullptr;
  void *d_ws = nullptr, *d_faces = nullptr;
  int32_t *d_walk = nullptr;  // the walker records of a chunk's strip or grid triples
  uint64_t *d_slots = nullptr;
  if (hipStreamCreateWithFlags(&B.s, hipStreamNonBlocking) != hipSuccess) return TSA_EDEVICE;
  if (!B.alloc(&d_seqs, max_seq) || !B.alloc(&d_moves, max_seq) ||
      !B.alloc(&d_meta, sizeof(int64_t) * (6 * (size_t)max_n + 1)) || !B.alloc(&d_slots, sizeof(uint64_t) * max_slots) ||
      !B.alloc(&d_res, sizeof(int32_t) * 12 * (size_t)max_n) || !B.alloc(&d_tb, max_cube) ||
      !B.alloc(&d_ws, max_ws) || !B.alloc(&d_faces, max_face) ||
      !B.alloc(&d_walk, pl.mode == ALIGN_MODE_STRIP || pl.mode == ALIGN_MODE_GRID
                            ? sizeof(int32_t) * ALIGN_WALK_REC * (size_t)max_n
                            : 0))
    return TSA_ENOMEM;
  std::vector<uint8_t> h_seqs(max_seq), h_moves(max_seq);
  std::vector<int64_t> h_meta(6 * (size_t)max_n + 1);
  std::vector<int32_t> h_res(12 * (size_t)max_n), order((size_t)max_n);
  for (const AlignChunk &c : chunks) {
    // launch order: resident triples first, then the over-capacity ones
    const int32_t m = c.i1 - c.i0, mr = m - c.n_over;
    int32_t r = 0, v = mr;
    for (int32_t i = c.i0; i < c.i1; ++i) order[T[i].over ? v++ : r++] = i;
    int64_t pos = 0, word = 0, cells = 0, keys = 0;
    int64_t *h_off = h_meta.data(), *h_tboff = h_meta.data() + 3 * (size_t)m + 1, *h_faceoff = h_tboff + m;
    int64_t *h_slotoff = h_faceoff + m;
    for (int32_t j = 0; j < m; ++j) {
      const AlignTriple &t = T[order[j]];
      std::memcpy(h_seqs.data() + pos, seqs + offsets[3 * (int64_t)order[j]], (size_t)t.la + t.lb + t.lc);
      h_off[3 * j] = pos, h_off[3 * j + 1] = pos + t.la, h_off[3 * j + 2] = pos + t.la + t.lb;
      pos += (int64_t)t.la + t.lb + t.lc;
      h_tboff[j] = word;
      word += (int64_t)(t.cube / sizeof(uint32_t));
      h_faceoff[j] = cells;
      if (c.tiled || c.strip || c.grid) cells += (int64_t)t.face;
      h_slotoff[j] = keys;
      if (keyed && c.grid && t.over) keys += (int64_t)t.nty * t.ntz;
    }
    h_off[3 * m] = pos;
    AlignDev d;
    d.seqs = d_seqs, d.off = d_meta, d.tboff = d_meta + 3 * (size_t)m + 1, d.faceoff = d.tboff + m;
    d.scores = d_res, d.final7 = d_res + m, d.info = d_res + 8 * (size_t)m;
    d.moves = d_moves, d.tb = d_tb, d.faces = d_faces, d.ws = d_ws, d.walk = d_walk;
    d.endrec = d.final7;
    d.slots = d_slots, d.slotoff = d.faceoff + m;
    if (hipMemcpyAsync(d_seqs, h_seqs.data(), (size_t)pos, hipMemcpyHostToDevice, B.s) != hipSuccess ||
        hipMemcpyAsync(d_meta, h_meta.data(), sizeof(int64_t) * (6 * (size_t)m + 1), hipMemcpyHostToDevice, B.s) !=
            hipSuccess)
      return TSA_EDEVICE;
    if ((rc = align_queue_chunk(c, pl, kp, d, B.s))) return rc;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h_res.data(), d_res, sizeof(int32_t) * 12 * (size_t)m, hipMemcpyDeviceToHost, B.s) !=
            hipSuccess ||
        hipMemcpyAsync(h_moves.data(), d_moves, (size_t)pos, hipMemcpyDeviceToHost, B.s) != hipSuccess ||
        hipStreamSynchronize(B.s) != hipSuccess)
      return TSA_EDEVICE;
    for (int32_t j = 0; j < m; ++j) {
      const int32_t i = order[j];
      const int32_t *info = h_res.data() + 8 * (size_t)m + 4 * (size_t)j;
      const int64_t len = offsets[3 * (int64_t)i + 3] - offsets[3 * (int64_t)i];
      if (info[0] < 1 || info[0] > len) return TSA_EINTERNAL;
      if (ends) {
        const AlignTriple &t = T[i];
        const int32_t *rec = h_res.data() + m + (size_t)ALIGN_END_REC * j;  // on final7, see AlignDev
        const int32_t corner[3] = {t.la, t.lb, t.lc};
        const int32_t *e = pl.end_mode != TSA_END_CORNER ? rec : corner;
        for (int k = 0; k < 3; ++k) ends[3 * (int64_t)i + k] = e[k];
      }
      std::memcpy(moves + (offsets[3 * (int64_t)i] - offsets[0]), h_moves.data() + h_off[3 * j], (size_t)info[0]);
      scores[i] = h_res[j];
      n_moves[i] = info[0];
      starts[3 * (int64_t)i] = info[1], starts[3 * (int64_t)i + 1] = info[2], starts[3 * (int64_t)i + 2] = info[3];
    }
  }
  return TSA_OK;
}

// ---- tsa_align_batch_async: the same plan against a caller's workspace -----
constexpr size_t kAlign256 = 256;
inline size_t up256(size_t v) { return (v + kAlign256 - 1) & ~(kAlign256 - 1); }

// The fixed part of the workspace, sized for the whole call from n, the total
// of symbols L and whether the path keeps walker records: byte offsets of its
// regions, each 256-byte aligned, and `total`, where the faces and cubes of a
// chunk begin. Chunk [i0, i1) uses entries i0.. of every per-triple region and
// the bytes of its triples in seqs and moves; its 3m+1 packed offsets start at
// entry 3*i0 + (index of the chunk), so off holds 3n + (chunks <= n) entries.
// keyed (tsa_align_batch_ends_async on the grid path with a free end): n slot
// offsets and the `keys` end keys of the call's grid triples, one per tile; a
// chunk uses the key region from its start. Both are empty otherwise.
struct AlignFixed {
  size_t seqs, moves, off, tboff, faceoff, order, scores, final7, info, walk, slotoff, slots, total;
};
AlignFixed align_fixed_layout(int32_t n, size_t L, bool walk, bool keyed = false, size_t keys = 0) {
  AlignFixed f;
  size_t at = 0;
  const auto take = [&](size_t bytes) {
    const size_t here = at;
    at += up256(bytes);
    return here;
  };
  f.seqs = take(L), f.moves = take(L);
  f.off = take(sizeof(int64_t) * 4 * (size_t)n);
  f.tboff = take(sizeof(int64_t) * (size_t)n), f.faceoff = take(sizeof(int64_t) * (size_t)n);
  f.order = take(sizeof(int32_t) * (size_t)n), f.scores = take(sizeof(int32_t) * (size_t)n);
  f.final7 = take(sizeof(int32_t) * NSTATE * (size_t)n), f.info = take(sizeof(int32_t) * 4 * (size_t)n);
  f.walk = take(walk ? sizeof(int32_t) * ALIGN_WALK_REC * (size_t)n : 0);
  f.slotoff = take(keyed ? sizeof(int64_t) * (size_t)n : 0), f.slots = take(keyed ? sizeof(uint64_t) * keys : 0);
  f.total = at;
  return f;
}

// What tsa_align_workspace_size prices and tsa_align_batch_async runs: the
// validated plan of a batch. cap: the budget of a chunk at most (align_tb_bytes).
struct AlignAsyncPlan {
  AlignPlan pl;
  std::vector<AlignTriple> T;
  AlignFixed fixed;
  size_t max_need = 0, cap = SIZE_MAX;
};
// end_mode = TSA_END_FACE / TSA_END_ANY (tsa_align_batch_ends_async): the plan
// of align_batch_entry's free end -- tiled or grid, no strips -- and on the
// grid path the key slots in the fixed part.
int align_async_plan(const int64_t *h_offsets, int32_t n, const tsa_params *p, int32_t path, AlignAsyncPlan *A,
                     int32_t end_mode = TSA_END_CORNER) {
  if (!h_offsets || n < 0 || !params_ok(p)) return TSA_EINVAL;
  if (end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY) return TSA_EINVAL;
  if (path != TSA_ALIGN_PATH_TILED && path != TSA_ALIGN_PATH_STRIP && path != TSA_ALIGN_PATH_GRID) return TSA_EINVAL;
  for (int32_t i = 0; i < n; ++i) {
    const int64_t *o = h_offsets + 3 * (int64_t)i;
    if (o[1] <= o[0] || o[2] <= o[1] || o[3] <= o[2] || o[3] - o[0] > INT32_MAX) return TSA_EINVAL;
  }
  int rc = align_plan_read(&A->pl);
  if (rc) return rc;
  if (!A->pl.mode_set)
    A->pl.mode = path == TSA_ALIGN_PATH_STRIP ? ALIGN_MODE_STRIP : path == TSA_ALIGN_PATH_GRID ? ALIGN_MODE_GRID
                                                                                               : ALIGN_MODE_TILED;
  else if (A->pl.mode != ALIGN_MODE_TILED && A->pl.mode != ALIGN_MODE_STRIP && A->pl.mode != ALIGN_MODE_GRID)
    return TSA_EINVAL;  // no resident-or-plane plan and no plane sweep on this path
  if (end_mode != TSA_END_CORNER && (path == TSA_ALIGN_PATH_STRIP || A->pl.mode == ALIGN_MODE_STRIP))
    return TSA_EINVAL;  // no end search on the strip path
  A->pl.end_mode = end_mode;
  long ov = 0;
  if (override_int("align_tb_bytes", &ov)) {
    if (ov < 0) return TSA_EINVAL;
    A->cap = (size_t)ov;
  }
  A->T = align_plan_triples(h_offsets, n, A->pl, true);
  for (const AlignTriple &t : A->T) A->max_need = std::max(A->max_need, t.need);
  const bool keyed = end_mode != TSA_END_CORNER && A->pl.mode == ALIGN_MODE_GRID;
  size_t keys = 0;  // whatever the chunks: every over-capacity triple is a grid triple of its chunk
  if (keyed)
    for (const AlignTriple &t : A->T) keys += t.over ? (size_t)t.nty * t.ntz : 0;
  A->fixed = align_fixed_layout(n, n ? (size_t)(h_offsets[3 * (int64_t)n] - h_offsets[0]) : 0,
                                A->pl.mode == ALIGN_MODE_STRIP || A->pl.mode == ALIGN_MODE_GRID, keyed, keys);
  return TSA_OK;
}

// What tsa_align_workspace_size and tsa_align_ends_workspace_size return for plan A.
int align_async_sizes(const AlignAsyncPlan &A, size_t *min_bytes, size_t *full_bytes) {
  *min_bytes = *full_bytes = 0;
  if (A.T.empty()) return TSA_OK;
  // the fewest chunks: the budget bounds none (but align_tb_bytes), only the 65535 triples of a chunk do
  std::vector<AlignChunk> chunks;
  int rc = align_plan_chunks(A.T, A.pl, A.cap, &chunks);
  if (rc) return rc;
  size_t most = 0;
  for (const AlignChunk &c : chunks) most = std::max(most, c.need);
  *min_bytes = A.fixed.total + A.max_need;
  *full_bytes = A.fixed.total + most;
  return TSA_OK;
}

// tsa_align_batch_async and tsa_align_batch_ends_async (d_ends set) behind
// their argument checks: the chunks of plan A against the workspace, launches only.
int align_async_run(const AlignAsyncPlan &A, const uint8_t *d_seqs, const int64_t *d_offsets, const int64_t *h_offsets,
                    const tsa_params *p, int32_t *d_scores, uint8_t *d_moves, int32_t *d_n_moves, int32_t *d_starts,
                    int32_t *d_ends, void *d_workspace, size_t workspace_bytes, void *stream) {
  if (tsa_device_count() <= 0) return TSA_ENODEV;
  KParams kp;
  int rc = build_kparams(p, &kp);
  if (rc) return rc;
  const bool free_end = A.pl.end_mode != TSA_END_CORNER, keyed = free_end && A.pl.mode == ALIGN_MODE_GRID;
  if (free_end)
    for (const AlignTriple &t : A.T)  // as align_batch_entry: far beyond any device's memory
      if (!align_end_key_fits(t.la, t.lb, t.lc)) return TSA_ENOMEM;
  if (workspace_bytes < A.fixed.total || workspace_bytes - A.fixed.total < A.max_need) return TSA_ENOMEM;
  std::vector<AlignChunk> chunks;
  if ((rc = align_plan_chunks(A.T, A.pl, std::min(workspace_bytes - A.fixed.total, A.cap), &chunks))) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint8_t *w = (uint8_t *)d_workspace;
  const AlignFixed &f = A.fixed;
  (void)hipGetLastError();  // an error left over from an earlier call is not this call's
  for (size_t k = 0; k < chunks.size(); ++k) {
    const AlignChunk &c = chunks[k];
    const int32_t m = c.i1 - c.i0;
    const size_t sym0 = (size_t)(h_offsets[3 * (int64_t)c.i0] - h_offsets[0]);  // the chunk's place in seqs and moves
    AlignChunkBufs b;
    b.off = (int64_t *)(w + f.off) + 3 * (size_t)c.i0 + k;
    b.tb_off = (int64_t *)(w + f.tboff) + c.i0, b.face_off = (int64_t *)(w + f.faceoff) + c.i0;
    b.order = (int32_t *)(w + f.order) + c.i0, b.scores = (int32_t *)(w + f.scores) + c.i0;
    b.final7 = (int32_t *)(w + f.final7) + (size_t)NSTATE * c.i0, b.info = (int32_t *)(w + f.info) + 4 * (size_t)c.i0;
    b.seqs = w + f.seqs + sym0, b.moves = w + f.moves + sym0;
    // the chunk's ALIGN_END_REC <= NSTATE words a triple on its part of final7; its keys from the region's start
    b.endrec = free_end ? b.final7 : nullptr;
    b.slot_off = keyed ? (int64_t *)(w + f.slotoff) + c.i0 : nullptr;
    AlignDev d;
    d.seqs = b.seqs, d.off = b.off, d.tboff = b.tb_off, d.faceoff = b.face_off;
    d.scores = b.scores, d.final7 = b.final7, d.info = b.info, d.moves = b.moves;
    // the faces (16-byte cells) first, then the cubes (words): c.face + c.cube = c.need bytes
    d.faces = w + f.total, d.tb = (uint32_t *)(w + f.total + c.face), d.ws = nullptr;
    d.walk = (int32_t *)(w + f.walk) + (size_t)ALIGN_WALK_REC * c.i0;
    d.endrec = b.endrec, d.slots = keyed ? (uint64_t *)(w + f.slots) : nullptr, d.slotoff = b.slot_off;
    align_launch_meta(d_offsets, c.i0, m, A.pl, b, s);
    align_launch_pack(d_seqs, d_offsets, m, b, s);
    if ((rc = align_queue_chunk(c, A.pl, kp, d, s))) return rc;
    align_launch_finish(d_offsets, m, b, d_scores, d_moves, d_n_moves, d_starts, s, d_ends);
  }
  return hipGetLastError() == hipSuccess ? TSA_OK : TSA_EDEVICE;
}
}  // namespace

extern "C" {

int tsa_describe_align_plan(int32_t n, int32_t la, int32_t lb, int32_t lc, const tsa_params *p, char *buf,
                            size_t len) {
  if (!buf || len == 0 || n < 1 || la < 1 || lb < 1 || lc < 1 || !params_ok(p)) return TSA_EINVAL;
  AlignPlan pl;
  int rc = align_plan_read(&pl);
  if (rc) return rc;
  switch (align_path(pl, la, lb, lc, n)) {
    case ALIGN_RESIDENT:
      snprintf(buf, len, "resident lds=%zu", align_resident_lds(la, lb, lc));
      break;
    case ALIGN_TILED: {
      const AlignTileGeom g = align_tile_geom(lb, lc, pl.tymax, pl.tzmax);
      snprintf(buf, len, "tiled tile=%dx%d tiles=%dx%d lds=%zu faces=%zu", g.TY, g.TZ, g.nty, g.ntz,
               align_resident_lds(la, g.TY, g.TZ), 16 * align_tiled_face_cells(la, lb, lc, pl.tymax, pl.tzmax));
      break;
    }
    case ALIGN_STRIP: {
      const AlignTileGeom g = align_tile_geom(lb, lc, pl.tymax, pl.tzmax);
      snprintf(buf, len, "strip tile=%dx%d tiles=%dx%d lds=%zu cube=%zu faces=%zu", g.TY, g.TZ, g.nty, g.ntz,
               align_resident_lds(la, g.TY, g.TZ), align_strip_cube_bytes(la, lb, lc, pl.tymax, pl.tzmax),
               16 * align_strip_face_cells(la, lb, lc, pl.tymax, pl.tzmax));
      break;
    }
    case ALIGN_GRID: {
      const AlignTileGeom g = align_tile_geom(lb, lc, pl.tymax, pl.tzmax);
      snprintf(buf, len, "grid tile=%dx%d tiles=%dx%d lds=%zu cube=%zu faces=%zu", g.TY, g.TZ, g.nty, g.ntz,
               align_resident_lds(la, g.TY, g.TZ), align_grid_cube_bytes(la, lb, lc, pl.tymax, pl.tzmax),
               16 * align_grid_face_cells(la, lb, lc, pl.tymax, pl.tzmax));
      break;
    }
    default:
      snprintf(buf, len, "plane");
  }
  return TSA_OK;
}

}  // extern "C"

namespace {
// tsa_align_batch, tsa_align_batch_lowmem and tsa_align_batch_grid:
// validation, plan, budget, run. unset: the plan mode unless align_mode is set
// (auto, strip under lowmem, grid).
// tsa_align_batch_ends: the same with end_mode and ends (null elsewhere).
int align_batch_entry(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p, int32_t *scores,
                      uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t device, AlignMode unset,
                      int32_t end_mode = TSA_END_CORNER, int32_t *ends = nullptr) {
  if (!seqs || !offsets || !scores || !moves || !n_moves || !starts || n < 0 || !params_ok(p)) return TSA_EINVAL;
  for (int32_t i = 0; i < n; ++i) {
    const int64_t *o = offsets + 3 * (int64_t)i;
    if (o[1] < o[0] || o[2] < o[1] || o[3] < o[2]) return TSA_EINVAL;
    int rc = tsa_validate(seqs + o[0], (int32_t)(o[1] - o[0]), seqs + o[1], (int32_t)(o[2] - o[1]),
                          seqs + o[2], (int32_t)(o[3] - o[2]), p);
    if (rc) return rc;
  }
  if (n == 0) return TSA_OK;
  AlignPlan pl;
  int rc = TSA_OK;
  if (end_mode != TSA_END_CORNER) {
    // the end search is the resident and the tiled kernel's, and the grid
    // kernels' under tsa_align_batch_grid_ends (unset = grid) alone: no plane
    // sweep, no strips -- a matter of the arguments, so it is found without a device
    if ((rc = align_plan_read(&pl))) return rc;
    if (pl.mode == ALIGN_MODE_PLANE || pl.mode == ALIGN_MODE_STRIP ||
        (pl.mode == ALIGN_MODE_GRID && unset != ALIGN_MODE_GRID))
      return TSA_EINVAL;
  }
  const int nd = tsa_device_count();
  if (nd <= 0) return TSA_ENODEV;
  if (device < 0 || device >= nd) return TSA_ENODEV;
  KParams kp;
  if ((rc = build_kparams(p, &kp))) return rc;
  if ((rc = align_plan_read(&pl))) return rc;
  if (!pl.mode_set) pl.mode = unset;
  pl.end_mode = end_mode;
  if (end_mode != TSA_END_CORNER)
    for (int32_t i = 0; i < n; ++i) {  // a cube the key cannot number is far beyond any device's memory
      const int64_t *o = offsets + 3 * (int64_t)i;
      if (!align_end_key_fits((int32_t)(o[1] - o[0]), (int32_t)(o[2] - o[1]), (int32_t)(o[3] - o[2]))) return TSA_ENOMEM;
    }
  if (hipSetDevice(device) != hipSuccess) return TSA_EDEVICE;
  // The pointer-cube budget of a chunk: align_tb_bytes, or half of the device
  // memory free at the call (the other half is left to the caller's own
  // buffers and to the sequences, moves, plane rings and tile faces of the
  // chunk, all of which are O(N^2) against the cubes' O(N^3)). On the strip
  // path a triple counts with its strip cube and its kept faces, on the grid
  // path with its tile cube and its kept faces.
  size_t budget = 0;
  long ov = 0;
  if (override_int("align_tb_bytes", &ov)) {
    if (ov < 0) return TSA_EINVAL;
    budget = (size_t)ov;
  } else {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return TSA_EDEVICE;
    budget = free_b / 2;
  }
  return align_run(seqs, offsets, n, kp, pl, budget, scores, moves, n_moves, starts, ends);
}
}  // namespace

extern "C" {

int tsa_align_batch(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p,
                    int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t device) {
  return align_batch_entry(seqs, offsets, n, p, scores, moves, n_moves, starts, device, ALIGN_MODE_AUTO);
}

int tsa_align_batch_lowmem(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p,
                           int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t device) {
  return align_batch_entry(seqs, offsets, n, p, scores, moves, n_moves, starts, device, ALIGN_MODE_STRIP);
}

int tsa_align_batch_grid(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p,
                         int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t device) {
  return align_batch_entry(seqs, offsets, n, p, scores, moves, n_moves, starts, device, ALIGN_MODE_GRID);
}

int tsa_align_batch_ends(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p, int32_t end_mode,
                         int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts, int32_t *ends,
                         int32_t device) {
  if (!ends || end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY) return TSA_EINVAL;
  return align_batch_entry(seqs, offsets, n, p, scores, moves, n_moves, starts, device, ALIGN_MODE_AUTO, end_mode, ends);
}

int tsa_align_batch_grid_ends(const uint8_t *seqs, const int64_t *offsets, int32_t n, const tsa_params *p,
                              int32_t end_mode, int32_t *scores, uint8_t *moves, int32_t *n_moves, int32_t *starts,
                              int32_t *ends, int32_t device) {
  if (!ends || end_mode < TSA_END_CORNER || end_mode > TSA_END_ANY) return TSA_EINVAL;
  return align_batch_entry(seqs, offsets, n, p, scores, moves, n_moves, starts, device, ALIGN_MODE_GRID, end_mode, ends);
}

int tsa_align_workspace_size(const int64_t *h_offsets, int32_t n, const tsa_params *p, int32_t path,
                             size_t *min_bytes, size_t *full_bytes) {
  if (!min_bytes || !full_bytes) return TSA_EINVAL;
  AlignAsyncPlan A;
  int rc = align_async_plan(h_offsets, n, p, path, &A);
  if (rc) return rc;
  return align_async_sizes(A, min_bytes, full_bytes);
}

int tsa_align_ends_workspace_size(const int64_t *h_offsets, int32_t n, const tsa_params *p, int32_t path,
                                  int32_t end_mode, size_t *min_bytes, size_t *full_bytes) {
  if (!min_bytes || !full_bytes) return TSA_EINVAL;
  AlignAsyncPlan A;
  int rc = align_async_plan(h_offsets, n, p, path, &A, end_mode);
  if (rc) return rc;
  return align_async_sizes(A, min_bytes, full_bytes);
}

int tsa_align_batch_async(const uint8_t *d_seqs, const int64_t *d_offsets, const int64_t *h_offsets, int32_t n,
                          const tsa_params *p, int32_t path, int32_t *d_scores, uint8_t *d_moves, int32_t *d_n_moves,
                          int32_t *d_starts, void *d_workspace, size_t workspace_bytes, void *stream) {
  if (!d_seqs || !d_offsets || !d_scores || !d_moves || !d_n_moves || !d_starts || !d_workspace) return TSA_EINVAL;
  if ((uintptr_t)d_workspace % kAlign256) return TSA_EINVAL;
  AlignAsyncPlan A;
  int rc = align_async_plan(h_offsets, n, p, path, &A);
  if (rc) return rc;
  if (n == 0) return TSA_OK;
  return align_async_run(A, d_seqs, d_offsets, h_offsets, p, d_scores, d_moves, d_n_moves, d_starts, nullptr,
                         d_workspace, workspace_bytes, stream);
}

int tsa_align_batch_ends_async(const uint8_t *d_seqs, const int64_t *d_offsets, const int64_t *h_offsets, int32_t n,
                               const tsa_params *p, int32_t path, int32_t end_mode, int32_t *d_scores,
                               uint8_t *d_moves, int32_t *d_n_moves, int32_t *d_starts, int32_t *d_ends,
                               void *d_workspace, size_t workspace_bytes, void *stream) {
  if (!d_seqs || !d_offsets || !d_scores || !d_moves || !d_n_moves || !d_starts || !d_ends || !d_workspace)
    return TSA_EINVAL;
  if ((uintptr_t)d_workspace % kAlign256) return TSA_EINVAL;
  AlignAsyncPlan A;
  int rc = align_async_plan(h_offsets, n, p, path, &A, end_mode);
  if (rc) return rc;
  if (n == 0) return TSA_OK;
  return align_async_run(A, d_seqs, d_offsets, h_offsets, p, d_scores, d_moves, d_n_moves, d_starts, d_ends,
                         d_workspace, workspace_bytes, stream);
}

int tsa_align_rows_async(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, const uint8_t *d_moves,
                         const int32_t *d_n_moves, const int32_t *d_starts, uint8_t *d_rows, void *stream) {
  if (!d_seqs || !d_offsets || !d_moves || !d_n_moves || !d_starts || !d_rows || n < 0) return TSA_EINVAL;
  if (n == 0) return TSA_OK;
  if (tsa_device_count() <= 0) return TSA_ENODEV;
  (void)hipGetLastError();
  align_launch_rows(d_seqs, d_offsets, n, d_moves, d_n_moves, d_starts, d_rows, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? TSA_OK : TSA_EDEVICE;
}

// One triple, always by the plane sweep, with buffers and a one-thread walk of
// its own: it reads no override and has no cube budget. As a batch of one
// through align_run it measured 0.1-0.3 ms slower per call.
int tsa_align_gpu(const uint8_t *a, int32_t la, const uint8_t *b, int32_t lb, const uint8_t *c,
                  int32_t lc, const tsa_params *p, int32_t *score, uint8_t *moves, int32_t max_moves,
                  int32_t *n_moves, int32_t *start, int32_t device) {
  if (!score || !moves || !n_moves || !start) return TSA_EINVAL;
  int rc = tsa_validate(a, la, b, lb, c, lc, p);
  if (rc) return rc;
  if ((int64_t)max_moves < (int64_t)la + lb + lc) return TSA_EINVAL;
  const int nd = tsa_device_count();
  if (nd <= 0) return TSA_ENODEV;
  if (device < 0 || device >= nd) return TSA_ENODEV;
  KParams kp;
  if ((rc = build_kparams(p, &kp))) return rc;
  const int64_t len = (int64_t)la + lb + lc;
  const int64_t off[4] = {0, la, (int64_t)la + lb, len};
  const size_t ws_bytes = plane_workspace_bytes(1, la, lb, lc);
  AlignBufs B;
  uint8_t *d_seqs = nullptr, *d_moves = nullptr;
  int64_t *d_off = nullptr;
  int32_t *d_small = nullptr, h_small[12];  // [0] score, [1..7] final states, [8..11] walk info
  uint32_t *d_tb = nullptr;
  void *d_ws = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&B.s, hipStreamNonBlocking) != hipSuccess)
    return TSA_EDEVICE;
  if (!B.alloc(&d_seqs, (size_t)len) || !B.alloc(&d_off, sizeof(off)) || !B.alloc(&d_small, sizeof(h_small)) ||
      !B.alloc(&d_moves, (size_t)len) || !B.alloc(&d_ws, ws_bytes) || !B.alloc(&d_tb, tb_cube_bytes(la, lb, lc)))
    return TSA_ENOMEM;
  if (hipMemcpyAsync(d_seqs, a, la, hipMemcpyHostToDevice, B.s) != hipSuccess ||
      hipMemcpyAsync(d_seqs + la, b, lb, hipMemcpyHostToDevice, B.s) != hipSuccess ||
      hipMemcpyAsync(d_seqs + la + lb, c, lc, hipMemcpyHostToDevice, B.s) != hipSuccess ||
      hipMemcpyAsync(d_off, off, sizeof(off), hipMemcpyHostToDevice, B.s) != hipSuccess)
    return TSA_EDEVICE;
  if ((rc = plane_launch_batch(d_seqs, d_off, 1, la, lb, lc, kp, d_small, d_small + 1, d_ws, ws_bytes, B.s, d_tb)))
    return rc;
  hipLaunchKernelGGL(tb_walk, dim3(1), dim3(64), 0, B.s, d_tb, d_small + 1, la, lb, lc, d_moves, d_small + 8);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(h_small, d_small, sizeof(h_small), hipMemcpyDeviceToHost, B.s) != hipSuccess ||
      hipStreamSynchronize(B.s) != hipSuccess)
    return TSA_EDEVICE;
  if (h_small[8] < 1 || h_small[8] > len) return TSA_EINTERNAL;
  std::vector<uint8_t> rev((size_t)h_small[8]);  // tb_walk gives the moves from the end backwards
  if (hipMemcpy(rev.data(), d_moves, rev.size(), hipMemcpyDeviceToHost) != hipSuccess) return TSA_EDEVICE;
  for (size_t k = 0; k < rev.size(); ++k) moves[k] = rev[rev.size() - 1 - k];
  *score = h_small[0];
  *n_moves = h_small[8];
  start[0] = h_small[9], start[1] = h_small[10], start[2] = h_small[11];
  return TSA_OK;
}

}  // extern "C"
