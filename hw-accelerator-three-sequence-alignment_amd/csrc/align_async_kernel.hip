// align_async_kernel.hip -- the helper kernels of the device-resident traceback
// entry points (align_api.hip): tsa_align_batch_async and
// tsa_align_batch_ends_async keep the caller's
// sequences, offsets and results on the device, so what align_run does on the
// host for the synchronous entry points around the traceback kernels is done
// here, in stream order:
//   align_meta_kernel    the metadata of a chunk -- packed offsets, cube and face
//                        offsets, the permutation back to the caller's index, and
//                        on the grid path with a free end the key slot offsets --
//                        from the caller's d_offsets (an upload from a host
//                        vector would make the call wait for the stream);
//   align_pack_kernel    the chunk's sequences packed in launch order (the
//                        traceback kernels take contiguous sub-batches);
//   align_finish_kernel  scores, starts, move counts and moves back to the
//                        caller's order and layout; its END form the end cells too;
//   align_rows_kernel    the three gapped rows of every alignment
//                        (tsa_align_rows_async).
// None of them waits for another workgroup: stream order is the only ordering.
//
// Traceback is an extension: the reference's alignment-output ports are
// commented out (src/TriAlign_tb.sv:239-260).

#include "align_kernel.h"

namespace tsa {

constexpr int META_NT = 256;

// One workgroup. Thread t owns the caller's triples [t*per, (t+1)*per) of the
// chunk: it sums what they need (pass 1), thread 0 scans the 256 sums, and the
// thread walks its triples again with the running values (pass 2). Launch
// order is a stable partition, the resident triples first: slot, packed
// position and cube word of a resident triple count the resident triples before
// it, those of an over-capacity one all resident triples and the over-capacity
// ones before it; face cells count over-capacity triples only. SLOTS (the grid
// path with a free end): the key slots as well, nty*ntz per over-capacity
// triple, counted like the face cells.
template <bool SLOTS>
__global__ __launch_bounds__(META_NT) void align_meta_kernel(const int64_t *__restrict__ offs, int32_t i0, int32_t m,
                                                             AlignPlan pl, AlignChunkBufs b) {
  __shared__ int64_t s_cnt[META_NT], s_len_r[META_NT], s_word_r[META_NT], s_len_o[META_NT], s_word_o[META_NT],
      s_cell_o[META_NT];
  __shared__ int64_t s_key_o[SLOTS ? META_NT : 1];
  __shared__ int64_t s_tot[3];  // resident triples, their symbols, their cube words
  const int tid = threadIdx.x;
  const int32_t per = (m + META_NT - 1) / META_NT;
  const int32_t j0 = tid * per < m ? tid * per : m, j1 = j0 + per < m ? j0 + per : m;
  const int64_t *o = offs + 3 * (int64_t)i0;
  for (int32_t k = tid; k < 4 * m; k += META_NT) b.info[k] = 0;
  int64_t cnt = 0, len_r = 0, word_r = 0, len_o = 0, word_o = 0, cell_o = 0, key_o = 0;
  // the key slots of an over-capacity triple: one per tile
  const auto keys = [&](int64_t lb, int64_t lc) {
    const AlignTileGeom g = align_tile_geom((int32_t)lb, (int32_t)lc, pl.tymax, pl.tzmax);
    return (int64_t)g.nty * g.ntz;
  };
  for (int32_t j = j0; j < j1; ++j) {
    const int64_t o0 = o[3 * (int64_t)j], o1 = o[3 * (int64_t)j + 1], o2 = o[3 * (int64_t)j + 2],
                  o3 = o[3 * (int64_t)j + 3];
    const AlignNeed t = align_need(pl, (int32_t)(o1 - o0), (int32_t)(o2 - o1), (int32_t)(o3 - o2));
    if (SLOTS && t.over) key_o += keys(o2 - o1, o3 - o2);
    if (t.over)
      len_o += o3 - o0, word_o += (int64_t)(t.cube / sizeof(uint32_t)), cell_o += (int64_t)t.face;
    else
      ++cnt, len_r += o3 - o0, word_r += (int64_t)(t.cube / sizeof(uint32_t));
  }
  s_cnt[tid] = cnt, s_len_r[tid] = len_r, s_word_r[tid] = word_r;
  s_len_o[tid] = len_o, s_word_o[tid] = word_o, s_cell_o[tid] = cell_o;
  if (SLOTS) s_key_o[tid] = key_o;
  __syncthreads();
  if (tid == 0) {  // exclusive scans of the 256 sums
    int64_t a = 0, c = 0, d = 0, e = 0, f = 0, g = 0, h = 0;
    for (int k = 0; k < META_NT; ++k) {
      int64_t v;
      if (SLOTS) v = s_key_o[k], s_key_o[k] = h, h += v;
      v = s_cnt[k], s_cnt[k] = a, a += v;
      v = s_len_r[k], s_len_r[k] = c, c += v;
      v = s_word_r[k], s_word_r[k] = d, d += v;
      v = s_len_o[k], s_len_o[k] = e, e += v;
      v = s_word_o[k], s_word_o[k] = f, f += v;
      v = s_cell_o[k], s_cell_o[k] = g, g += v;
    }
    s_tot[0] = a, s_tot[1] = c, s_tot[2] = d;
    b.off[3 * (int64_t)m] = c + e;
  }
  __syncthreads();
  int64_t slot_r = s_cnt[tid], pos_r = s_len_r[tid], wd_r = s_word_r[tid];
  int64_t slot_o = s_tot[0] + (j0 - s_cnt[tid]), pos_o = s_tot[1] + s_len_o[tid], wd_o = s_tot[2] + s_word_o[tid];
  int64_t cl_o = s_cell_o[tid], ky_o = SLOTS ? s_key_o[tid] : 0;
  for (int32_t j = j0; j < j1; ++j) {
    const int64_t o0 = o[3 * (int64_t)j], o1 = o[3 * (int64_t)j + 1], o2 = o[3 * (int64_t)j + 2],
                  o3 = o[3 * (int64_t)j + 3];
    const AlignNeed t = align_need(pl, (int32_t)(o1 - o0), (int32_t)(o2 - o1), (int32_t)(o3 - o2));
    const int64_t slot = t.over ? slot_o : slot_r, pos = t.over ? pos_o : pos_r;
    b.off[3 * slot] = pos, b.off[3 * slot + 1] = pos + (o1 - o0), b.off[3 * slot + 2] = pos + (o2 - o0);
    b.tb_off[slot] = t.over ? wd_o : wd_r;
    b.face_off[slot] = t.over ? cl_o : 0;
    b.order[slot] = i0 + j;
    if (SLOTS) {
      b.slot_off[slot] = t.over ? ky_o : 0;
      if (t.over) ky_o += keys(o2 - o1, o3 - o2);
    }
    if (t.over)
      ++slot_o, pos_o += o3 - o0, wd_o += (int64_t)(t.cube / sizeof(uint32_t)), cl_o += (int64_t)t.face;
    else
      ++slot_r, pos_r += o3 - o0, wd_r += (int64_t)(t.cube / sizeof(uint32_t));
  }
}

void align_launch_meta(const int64_t *d_offsets, int32_t i0, int32_t m, const AlignPlan &pl, const AlignChunkBufs &b,
                       hipStream_t stream) {
  if (b.slot_off)
    hipLaunchKernelGGL(align_meta_kernel<true>, dim3(1), dim3(META_NT), 0, stream, d_offsets, i0, m, pl, b);
  else
    hipLaunchKernelGGL(align_meta_kernel<false>, dim3(1), dim3(META_NT), 0, stream, d_offsets, i0, m, pl, b);
}

// Workgroup j: the symbols of launch slot j, from the caller's buffer to their
// packed place.
__global__ __launch_bounds__(256) void align_pack_kernel(const uint8_t *__restrict__ seqs,
                                                         const int64_t *__restrict__ offs, AlignChunkBufs b) {
  const int64_t j = blockIdx.x;
  const int64_t p0 = b.off[3 * j], len = b.off[3 * j + 3] - p0;
  const uint8_t *src = seqs + offs[3 * (int64_t)b.order[j]];
  uint8_t *dst = b.seqs + p0;
  for (int64_t k = threadIdx.x; k < len; k += blockDim.x) dst[k] = src[k];
}

void align_launch_pack(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t m, const AlignChunkBufs &b,
                       hipStream_t stream) {
  hipLaunchKernelGGL(align_pack_kernel, dim3(m), dim3(256), 0, stream, d_seqs, d_offsets, b);
}

// Workgroup (one wave) j: the results of launch slot j to the caller's index.
// Only the first n_moves bytes of the caller's slot are written. ENDS: the end
// cell as well, from the triple's end record, or its lengths when the chunk has
// no records (TSA_END_CORNER).
template <bool ENDS>
__global__ __launch_bounds__(64) void align_finish_kernel(const int64_t *__restrict__ offs, AlignChunkBufs b,
                                                          int32_t *__restrict__ scores, uint8_t *__restrict__ moves,
                                                          int32_t *__restrict__ n_moves,
                                                          int32_t *__restrict__ starts, int32_t *__restrict__ ends) {
  const int64_t j = blockIdx.x, i = b.order[j];
  const int64_t p0 = b.off[3 * j], len = b.off[3 * j + 3] - p0;
  const int32_t *info = b.info + 4 * j;
  const int32_t nm = info[0] >= 1 && info[0] <= len ? info[0] : 0;
  if (threadIdx.x == 0) {
    scores[i] = b.scores[j];
    n_moves[i] = nm;
    starts[3 * i] = info[1], starts[3 * i + 1] = info[2], starts[3 * i + 2] = info[3];
    if (ENDS) {
      if (b.endrec) {
        const int32_t *rec = b.endrec + (int64_t)ALIGN_END_REC * j;
        ends[3 * i] = rec[0], ends[3 * i + 1] = rec[1], ends[3 * i + 2] = rec[2];
      } else {
        const int64_t *o = offs + 3 * i;
        ends[3 * i] = (int32_t)(o[1] - o[0]), ends[3 * i + 1] = (int32_t)(o[2] - o[1]);
        ends[3 * i + 2] = (int32_t)(o[3] - o[2]);
      }
    }
  }
  const uint8_t *src = b.moves + p0;
  uint8_t *dst = moves + (offs[3 * i] - offs[0]);
  for (int32_t k = threadIdx.x; k < nm; k += 64) dst[k] = src[k];
}

void align_launch_finish(const int64_t *d_offsets, int32_t m, const AlignChunkBufs &b, int32_t *d_scores,
                         uint8_t *d_moves, int32_t *d_n_moves, int32_t *d_starts, hipStream_t stream,
                         int32_t *d_ends) {
  if (d_ends)
    hipLaunchKernelGGL(align_finish_kernel<true>, dim3(m), dim3(64), 0, stream, d_offsets, b, d_scores, d_moves,
                       d_n_moves, d_starts, d_ends);
  else
    hipLaunchKernelGGL(align_finish_kernel<false>, dim3(m), dim3(64), 0, stream, d_offsets, b, d_scores, d_moves,
                       d_n_moves, d_starts, d_ends);
}

// One wave per triple, 64 alignment columns per step. Column k of row r shows
// a symbol when move k consumes sequence r (the predecessor offsets of
// src/PE_1cyc.v:164-218, TSA_MOVE_*) and a gap when not. The index of that
// symbol is start[r] + the consuming columns before k: the consuming columns of
// earlier steps (run) plus the consuming lanes below this one, which is one
// ballot over the wave and an mbcnt of it -- no lane waits for another. An
// index outside the sequence (moves that do not belong to these sequences)
// reads nothing and shows a gap.
__global__ __launch_bounds__(64) void align_rows_kernel(const uint8_t *__restrict__ seqs,
                                                        const int64_t *__restrict__ offs,
                                                        const uint8_t *__restrict__ moves,
                                                        const int32_t *__restrict__ n_moves,
                                                        const int32_t *__restrict__ starts,
                                                        uint8_t *__restrict__ rows) {
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t o0 = offs[3 * i], o1 = offs[3 * i + 1], o2 = offs[3 * i + 2], o3 = offs[3 * i + 3];
  const int64_t base = o0 - offs[0], len = o3 - o0;
  int64_t nm = n_moves[i];
  nm = nm < 0 ? 0 : nm > len ? len : nm;
  const uint8_t *mv = moves + base;
  uint8_t *row = rows + 3 * base;
  // states {M,Ix,Iy,Iz,Ixy,Iyz,Ixz} that consume A, B, C, one bit per state
  const uint32_t eatA = 0x53u, eatB = 0x35u, eatC = 0x69u;
  int64_t runA = starts[3 * i], runB = starts[3 * i + 1], runC = starts[3 * i + 2];
  for (int64_t k0 = 0; k0 < nm; k0 += 64) {
    const int64_t k = k0 + lane;
    const bool on = k < nm;
    const uint32_t bit = on && mv[k] < 7 ? 1u << mv[k] : 0u;
    const auto put = [&](uint32_t eat, int64_t s0, int64_t ls, int64_t &run, uint8_t *out) {
      const bool eats = (bit & eat) != 0;
      const unsigned long long mask = __ballot(eats);
      const int64_t idx = run + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      if (on) out[k] = eats && idx >= 0 && idx < ls ? seqs[s0 + idx] : (uint8_t)TSA_ROW_GAP;
      run += __popcll(mask);
    };
    put(eatA, o0, o1 - o0, runA, row);
    put(eatB, o1, o2 - o1, runB, row + len);
    put(eatC, o2, o3 - o2, runC, row + 2 * len);
  }
}

void align_launch_rows(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, const uint8_t *d_moves,
                       const int32_t *d_n_moves, const int32_t *d_starts, uint8_t *d_rows, hipStream_t stream) {
  hipLaunchKernelGGL(align_rows_kernel, dim3(n), dim3(64), 0, stream, d_seqs, d_offsets, d_moves, d_n_moves, d_starts,
                     d_rows);
}

}  // namespace tsa
