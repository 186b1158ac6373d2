// pencil_kernel.hip -- TSA_KERNEL_PENCIL: register-systolic 3-D DP for CDNA4.
//
// The reference computes the cube with an 8x8 systolic PE array over (y,z)
// while A streams along x (src/TriAlign_1cyc.v:115-125, PE_1cyc.v:247-299),
// slicing the (y,z) plane into 8x8 pencils with face SRAMs between them
// (src/TriAlign_1cyc.v:78-98). This kernel keeps that idea -- every cell is
// computed from neighbour values that arrive by systolic shifts, never from a
// stored cube -- but shapes it for a 64-lane wave:
//
//  * one workgroup scores one triple; wave w of NW owns DP row y = lap*NW+w+1;
//  * the 64 lanes x M packed int16 pairs own Zt = 128*M consecutive z
//    positions k (lane l, register i, half h -> k = 64Mh + Ml + i), z = k+1:
//    a lane's consecutive positions sit in consecutive registers;
//  * position k of wave w computes cell x = u mod P + 1 of lap u div P at step
//    t, with u = t - w - k (one step of skew per y and per z). A lane that
//    finishes x = P of lap L continues with x = 1 of lap L+1 (row y+NW), so
//    there is no fill/drain between rows: the positions form a helix;
//  * z-1 neighbours arrive by register renaming (i >= 1) and one DPP
//    wave_ror:1 + v_perm for register 0, per message and step whatever M is,
//    y-1 neighbours through a 2-slot LDS record per wave pair, and the wave
//    above wave 0 (row y-1 of the previous lap) through a global ring that the
//    last wave writes and wave 0 prefetches PD steps ahead with LDS-DMA;
//  * A, B and the "x == 1" position flow through the same shifts; only lane
//    0 of pair 0 gets injected values (the z = 0 face, the next A symbol and
//    the current B symbol).
//
// Arithmetic is the factored ("message") form of src/PE_1cyc.v:164-218: a
// cell sends to each successor target T the value max_s(S[s] - P[T][s]) and
// the successor adds its pair/triple score. It equals the RTL's literal
// 49-candidate MAX7 whenever no candidate wraps at SCORE_BITS and every value
// fits int16, which the host proves a priori (trialign_api.hip:pencil_exact)
// before it ever selects this kernel.
//
// Supported shapes: LC <= 128*M (M = 1 or 2), LA <= 4096, LB <= 4096.


// The step (the `step` lambda of pencil_kernel), in the order it executes. One
// form of each part exists; where the forms differ between instantiations the
// condition is a shape (the constexpr names RP, FIRSTLAP, A_EVEN, A_B64,
// MASK_PAIRS, HSK), never a build choice. What each form replaced, and the
// forms that were built, measured and taken out again, are in DESIGN.md 4.2, 8
// and Appendix H.
//
//  1. A codes. V-space: from registers an even step filled for itself's two
//     successors (for M = 2 as one ds_read_b64 each, from the table or its copy
//     shifted by one entry), so no LDS read is pending at an odd step's barrier.
//     Other forms: read by the step before, ahead of its barrier.
//  2. Record of the wave above. RP (V-space M = 2, one triple, skew 2): {Iy,
//     Ixy} from the lane's own record, {Iyz, best} from position k - 1's, by the
//     address of the read (read_prev); other forms read their own record and
//     shift it in step 7. Wave 0 reads the ring rows prefetched into xr0; in
//     V-space it builds the face records of its steps before t_sw from its own
//     H registers instead (ROLE 3), and the prologue fills only the ring rows
//     of steps [t_sw, lag).
//  3. x = 1 injection into the inputs: the half mask of the x = 1 position is
//     kept in a register and switched at two events per lap (hm_of / ev_of); the
//     lane's bfi mask is one v_cndmask, shared by a pair of steps
//     (MASK_PAIRS). The position takes the x = 0 faces, the row's B code (RP:
//     from the SGPR it lives in) and the per-row terms computed once per lap
//     (row_terms).
//  4. The cell: cell_messages{,_f16,_vs,_vi} at priority 0 between two
//     scheduling fences; the rest of the step runs at priority 1.
//  5. Final-cell capture, then the record send: one ds_write_b128 per register
//     to the wave below; the last wave stores to the ring row instead (RP: the
//     row's uniform base plus the lane's 32-bit offset, the store's saddr form)
//     and keeps at most STORE_SLACK steps of stores in flight.
//  6. END: the end search's fold of the step's real cells.
//  7. Advance: V-space sets H(t + 2); position 0 moves on, its half-mask and
//     lap-wrap events tested only at the one step of a four-step group where
//     they can fall (EV_SKIP; V-space M = 2, where P is a multiple of 4); the
//     own messages shift by DPP wave_ror:1 + v_perm (zshift), the row-above ones
//     likewise or, RP, by lane 0's v_perm alone (zfix).
//  8. V-space, even steps: the A reads of step 1.
//  9. Ring fetch. The RP forms: waves 1 and 2 issue wave 0's rows with
//     dma16x2_saddr at the even steps of their groups from group t_iss on, the
//     row of step t + 6 (wave 1) or t + 7 (wave 2), and wait with a counted
//     vmcnt at the odd steps until only their two newest rows are in flight;
//     the step barrier is the only synchronisation, and nothing is primed.
//     Other forms: wave 0 fetches its own row of step t + PD (prime() fills the
//     pipeline), for non-V-space M = 2 also through dma16x2_saddr.
// 10. s_waitcnt lgkmcnt(0) + s_barrier: every step at skew 1, every second
//     step at skew 2 (a wave reads records two steps old).

#include <vector>

#include "pencil_common.h"
#include "lap_kernel.h"

namespace tsa {


// waves (= DP rows) per lap: 8, two workgroups per CU, so one computes while
// the other waits at its barrier (16 waves, one workgroup per CU and half the
// ring traffic, measured 3 % slower: profiles/r6j_helix_nw16_ab.jsonl)
constexpr int PENCIL_NW = 8;
// the last wave keeps <= this many steps of ring stores in flight (a deeper
// slack, 8 or 16, measured neutral: DESIGN.md 4.2, "The ring's share")
constexpr int STORE_SLACK = 4;
constexpr int MAX_LA = 4096, MAX_LB = 4096, MAX_LC = 1024;
// LDS-DMA prefetch distance (steps) of wave 0: helix (ring) and lap (hand-off);
// shorter for wide positions (M pairs per lane) so the record slots fit in LDS
__host__ __device__ constexpr int helix_pd(int M) { return M >= 8 ? 2 : M >= 4 ? 4 : 8; }
// steps between waves, and record slots per wave: 2 up to M = 2, one barrier per
// two steps (1403-1465 -> 1476-1514 GCUPS over skew 1); M >= 4
// keeps skew 1 (twice the slots would not fit LDS)
__host__ __device__ constexpr int helix_skew(int M) { return M <= 2 ? 2 : 1; }
constexpr int RING_EXTRA = 8;
// v_bfi_b32 with an SGPR source for the selected bits
__device__ __forceinline__ uint32_t vbfi_s(uint32_t mask, uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "s"(a), "v"(b));
  return r;
}
// An M = 2 ring row's fetch as one statement: both 1 KiB pieces through the
// saddr form (the row's SGPR base, the lane's two constant VGPR offsets), M0 set
// from a 32-bit LDS address -- no per-step 64-bit VALU address, no generic-to-
// LDS pointer check, one M0 save / restore.
// (only s_mov in the statement: an s_add would write SCC behind the compiler's back)
__device__ __forceinline__ void dma16x2_saddr(const uint8_t *sbase, uint32_t voff0, uint32_t voff1,
                                              uint32_t lds0, uint32_t lds1) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3 sc1\n\t"
      "s_mov_b32 m0, %5\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %3 sc1\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff0), "v"(voff1), "s"(sbase), "s"(lds0), "s"(lds1)
      : "memory");
}
// A-table entries past P + 128M repeating its start (the table is periodic in
// P): the V-space loop reads a four-step group's A codes at constant offsets
// from one address computed at the group's start, across a lap wrap too
constexpr int A_PAD = 4;

struct PencilGeom {
  int32_t M;        // pairs per lane
  int32_t P;        // lap period (steps)
  int32_t R;        // ring rows
  bool two;         // two triples per workgroup (LC <= 64, M = 1)
  int64_t ring_bytes_per_triple;
};
// waves per CU the VGPR budget allows: 4 per SIMD up to M = 2, 2 beyond
static int waves_per_cu(int M) { return M >= 4 ? 8 : 16; }

static int helix_nw(int M) { return M == 2 ? PENCIL_NW : 8; }
// TWO: for LC <= 64 a wave's two 16-bit halves hold two different triples at
// the same 64 positions (a lane = one z of both), instead of positions k and
// k+64 of one triple -- no idle half, and the lap period shrinks to max(LA, 64).
static bool helix_two(int32_t max_lc) {
  long v = 0;
  if (override_int("pencil_two", &v)) return v != 0 && max_lc <= 64;  // plan override (A/B)
  return max_lc <= 64;
}
// no_two: the end search's geometry (a wave's two halves are one triple's)
static PencilGeom pencil_geom(int32_t max_la, int32_t max_lc, bool no_two = false) {
  PencilGeom g;
  g.M = pencil_pairs(max_lc);
  // >= 64 > NW + helix_pd + STORE_SLACK: ring lag
  g.two = !no_two && helix_two(max_lc);
  g.P = std::max(max_la, g.two ? 64 : 128 * g.M);
  g.P = (g.P + g.M - 1) / g.M * g.M;  // even for M = 2: the x = 1 register is PH ^ (w & 1)
  // M = 2: a multiple of 4, so the half-mask and lap-wrap events fall on one static
  // step of a wave's four-step group (EV_SKIP in step)
  if (g.M == 2 && !g.two) g.P = (g.P + 3) / 4 * 4;
  g.R = g.P + RING_EXTRA;
  g.ring_bytes_per_triple = (int64_t)g.R * g.M * 64 * REC_BYTES;
  return g;
}
// vs: the V-space instantiation, whose M = 2 form (A_B64) also keeps the
// A table's copy shifted by one entry after fin; the other forms do not
static size_t helix_lds(int M, int NW, int32_t P, int32_t max_lb, bool vs) {
  const size_t a_tab = 4 * ((size_t)P + 128 * M + A_PAD);
  return (size_t)(NW - 1) * 2 * helix_skew(M) * M * 1024 + (size_t)helix_pd(M) * M * 1024 + a_tab +
         4 * (((size_t)max_lb + 3) & ~(size_t)3) + (size_t)M * 512 + (vs && M == 2 ? a_tab : 0);
}

// The factored messages widen each target's highest-penalty group to all seven
// states, exact only when gap_open >= gap_extend (cell_messages_f16).
bool pencil_supported(const tsa_params *p) { return p != nullptr && p->gap_open >= p->gap_extend; }

static bool pencil_shape_ok(int32_t max_la, int32_t max_lb, int32_t max_lc) {
  if (!(max_la >= 1 && max_la <= MAX_LA && max_lb >= 1 && max_lb <= MAX_LB && max_lc >= 1 &&
        max_lc <= MAX_LC))
    return false;
  const PencilGeom g = pencil_geom(max_la, max_lc);
  // the helix is always runnable: the non-V-space form (use_vs admits the
  // V-space one only where its own footprint fits too)
  return helix_lds(g.M, helix_nw(g.M), g.P, max_lb, false) <= LDS_MAX;
}

static bool use_f16(const KParams &kp, const Range &r);
static bool use_vs(const KParams &kp, const Range &r, int32_t max_la, int32_t max_lb, int32_t max_lc);
static int32_t use_vi(const KParams &kp, const Range &r, int32_t max_la, int32_t max_lb, int32_t max_lc);

// Estimated latency (us) of the helix kernel for a batch: dispatch waves x
// steps per triple x step time. Measured: a fully loaded chip (two 8-wave
// workgroups per CU) runs an M = 2 step in ~0.66 us (512 x 256^3 in 5.6 ms);
// a workgroup alone on its CU in 0.38 us (one 256^3 triple, 3.2 ms), M = 1
// (two triples per wave) in 0.31 us (one 64^3 triple, 0.18 ms).
static double helix_step_us(int M, bool loaded) {
  const double s = M == 1 ? 0.40 : M == 2 ? 0.66 : M == 4 ? 1.2 : 2.4;
  const double alone = M == 1 ? 0.31 : M == 2 ? 0.38 : M == 4 ? 0.7 : 1.4;
  return loaded ? s : alone;
}
static double helix_est(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc) {
  const PencilGeom g = pencil_geom(max_la, max_lc);
  const int nw = helix_nw(g.M);
  const int64_t per_cu = std::max<int64_t>(
      1, std::min<int64_t>(LDS_MAX / helix_lds(g.M, nw, g.P, max_lb, g.M == 2), waves_per_cu(g.M) / nw));
  const double T = (double)((max_lb - 1) / nw) * g.P + max_la + nw + max_lc;
  const int64_t units = g.two ? (n + 1) / 2 : n;
  return (double)((units + 256 * per_cu - 1) / (256 * per_cu)) * T *
         helix_step_us(g.M, units > 256);
}

// The lap kernel's geometry if it should run, else .ok = false (helix).
// Resident grids (waves == 1) are safe: every workgroup runs at once, so a
// consumer waiting for a record never holds a slot its producer needs. A cube
// beyond the resident slots runs in rounds inside one resident grid: each
// workgroup loops over its slot's laps in lap order (lap_kernel), so a
// consumer's producer is always running or done, and a producer never waits
// for a consumer of a later round (boundary rings, lap_geom); every wait is
// bounded.
// ends: the end search's plan (lap_ends_kernel: int16, M <= 2, its own residency).
static LapGeom lap_choice(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc,
                          LapPolicy lap, bool f16, bool sop, bool need = false, bool ends = false) {
  LapGeom none{};
  none.ok = false;
  if (lap == LAP_OFF || max_la > 4096 || max_la + 2 * 8 + 64 * 4 >= 8192) return none;
  char mode[16] = "";  // plan overrides (tsa_set_override)
  override_str("pencil_mode", mode, sizeof mode);
  if (!strcmp(mode, "helix")) return none;
  const bool force = !strcmp(mode, "lap");
  int m_lo = 1, m_hi = 4, nw_lo = 4, nw_hi = 8;
  long v = 0;
  if (override_int("lap_m", &v)) m_lo = m_hi = (int)std::max(1L, std::min(4L, v));
  if (override_int("lap_nw", &v)) nw_lo = nw_hi = v == 4 ? 4 : 8;
  if (ends) m_hi = std::min(m_hi, 2);  // z tiles cover any LC at M <= 2
  LapGeom best = none;
  for (int M = m_lo; M <= m_hi; M *= 2) {
    for (int NW = nw_lo; NW <= nw_hi; NW *= 2) {
      // several rounds run as the resident workgroups' loops with boundary
      // rings (lap_geom), at any workgroups per CU (when the hardware
      // dispatcher ran round 2, two per CU started out of chain order and
      // timed out); a larger batch runs as chunks of triples, one launch
      // each (lap_geom_chunked)
      const LapGeom g = lap_geom_chunked(n, max_la, max_lb, max_lc, M, NW, f16, sop, false, ends);
      if (!g.ok) continue;
      if (!best.ok || g.est_us < best.est_us) best = g;
    }
  }
  // `need` (the checked kernel): the lap schedule whatever the helix would cost;
  // otherwise the lap must win by a margin (its estimate is ~10-30 % uncertain,
  // and the helix has no cross-workgroup dependency)
  if (best.ok && !force && !need && 1.25 * best.est_us >= helix_est(n, max_la, max_lb, max_lc)) return none;
  return best;
}

bool pencil_checked_plan(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc,
                         const KParams &kp, LapPolicy lap) {
  return pencil_shape_ok(max_la, max_lb, max_lc) &&
         lap_choice(n, max_la, max_lb, max_lc, lap, false, kp.s3_mode == TSA_S3_SOP, true).ok;
}

size_t pencil_workspace_bytes(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc,
                              const KParams &kp, const Range &bound, LapPolicy lap, bool checked) {
  if (checked) {
    const LapGeom g = lap_choice(n, max_la, max_lb, max_lc, lap, false, kp.s3_mode == TSA_S3_SOP, true);
    return g.ok ? lap_workspace_bytes(g) : 0;
  }
  if (!pencil_shape_ok(max_la, max_lb, max_lc)) return 0;
  const size_t helix = (size_t)std::min<int32_t>(n, 65535) *
                       (size_t)pencil_geom(max_la, max_lc).ring_bytes_per_triple;
  const LapGeom g = lap_choice(n, max_la, max_lb, max_lc, lap, use_f16(kp, bound),
                               kp.s3_mode == TSA_S3_SOP);
  if (g.ok) return std::max(helix, lap_workspace_bytes(g));
  return helix;
}

bool pencil_shape_supported(int32_t max_la, int32_t max_lb, int32_t max_lc) {
  return pencil_shape_ok(max_la, max_lb, max_lc);
}

// The end search's per-lane state (pencil_kernel END): the running key of each
// position (v[h][i]: half h of register i) and the lane's first position. Empty
// unless END: as plain locals the step lambda captures them, and unused they
// still cost every other instantiation a VGPR.
template <int M, bool END>
struct EndKeys {
  uint32_t v[2][M];
  uint32_t kl;
};
template <int M>
struct EndKeys<M, false> {};

// ---------------------------------------------------------------------------
// Helix kernel: one workgroup per triple (grid-stride over the batch).
//   LDS: xr  [NW-1][2][M][64][16]  wave w -> w+1 records {Iy, Ixy, Iyz, best}
//        xr0 [PD][M][64][16]       ring rows prefetched for wave 0 (LDS-DMA), PD = helix_pd(M)
//        sA2 [P+ZT] u32            A codes for positions k and k+64 of one pair
//        sB  [LB] u32              B code, both halves
//        fin [M][64] u32           best of the final step (wave w_f)
// F16 selects the exact-f16 arithmetic above, else the int16 form; VS the
// V-space f16 cell (cell_messages_vs): every value shifted by lam*(x+y+z), the
// zero faces injected as lam*q (x = 1: H(t), H(t-1); z = 0: H(t+1), H(t+2);
// y = 0: the ring's face records), the score shifted back at the end.
// VI: the V-space cell on integer bit patterns (cell_messages_vi): every half
// holds bias + 8 V, the symbol codes are 1 << s, the per-row terms integer
// weights. Records, ring, z-shifts and injections move bits and do not change.
// END: the end-free score (tsa_score_batch_ends): every step folds the real
// cells' MAX7 into one key per position and half (end_fold, pencil_common.h);
// the largest key gives scores[tri] and ends[3 tri ..] = (x1, y1, z1), and the
// corner's fin capture drops out. pa.end_face restricts the candidates
// to the three end faces (wave-uniform, tested once per step).
template <int M, int NW, bool F16, bool SOP, bool TWO, bool VS, bool VI = false, bool END = false>
__global__ __launch_bounds__(64 * NW) void pencil_kernel(const uint8_t *__restrict__ seqs,
                                                         const int64_t *__restrict__ offs,
                                                         int32_t n, int32_t P, int32_t R,
                                                         int32_t lds_a, int32_t lds_b,
                                                         int64_t ring_stride,
                                                         uint8_t *__restrict__ ring_base,
                                                         int32_t *__restrict__ scores,
                                                         PencilArgs pa, int32_t *__restrict__ ends) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int PAIR_BYTES = 64 * REC_BYTES;  // one pair's record, 1 KiB
  constexpr int SLOT_BYTES = M * PAIR_BYTES;
  constexpr int ZT = 128 * M;
  constexpr int PD = helix_pd(M);
  constexpr int HSK = helix_skew(M), HNSL = 2 * HSK;
  uint8_t *xr = smem;
  uint8_t *xr0 = xr + (NW - 1) * HNSL * SLOT_BYTES;
  uint32_t *sA2 = (uint32_t *)(xr0 + PD * SLOT_BYTES);
  uint32_t *sB = (uint32_t *)((uint8_t *)sA2 + lds_a);
  uint32_t *fin = (uint32_t *)((uint8_t *)sB + lds_b);
  uint32_t *sA2s = (uint32_t *)((uint8_t *)fin + M * 512);  // A_B64: sA2 shifted by one entry
  constexpr bool A_B64 = VS && M == 2;  // a step's A codes as one ds_read_b64 (load_a_pair)

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  static_assert(!TWO || M == 1, "two triples per wave: 64 positions, M = 1");
  static_assert(!VS || (F16 && M <= 2), "V-space: the f16 helix with the four-step loop");
  static_assert(!VI || (VS && M == 2 && !TWO && helix_skew(M) == 2),
                "integer patterns: the V-space M = 2 helix at skew 2");
  static_assert(!END || (F16 && !TWO && M <= 2), "end search: the f16-class helix, one triple per workgroup");
  constexpr uint32_t SYMC = VI ? 1u : SYM0;  // symbol codes SYMC << s
  // f16 bits of an integer (|v| <= 2048: exact), in both halves; VI: bias + 8 v
  auto h_bits = [&](int32_t v) -> uint32_t {
    if constexpr (VI) return (uint32_t)(pa.bias + 8 * v) * 0x00010001u;
    const _Float16 h = (_Float16)(float)v;
    return (uint32_t)__builtin_bit_cast(uint16_t, h) * 0x00010001u;
  };
  // per-half weight w / code of a one-hot code (the match bonus' multiplier)
  auto w_over_code = [&](float wf, int32_t w8, uint32_t codes) -> uint32_t {
    if constexpr (VI) return w8_over_code(w8, codes);
    else return dm_over_code(wf, codes);
  };
  // TWO: the halves are two triples at the same position, so lane 0 takes its
  // whole word from the z = 0 face (no half crosses from lane 63)
  const uint32_t sel = lane == 0 ? (TWO ? 0x03020100u : 0x05040302u) : 0x07060504u;
  constexpr int KS = TWO ? 64 : 128 * M;  // positions (per half in TWO)
  uint32_t ones = F16 ? 0x08000800u : 0x00010001u;  // f16: match indicator 2^-13
  asm volatile("" : "+v"(ones));                     // keep it in a VGPR (VOP3P operand)
  const PencilArgs pv = F16 ? pa : pin_score_consts(pa);
  uint32_t fsv = pa.f_single, fpv = pa.f_pair;  // VGPR copies for v_bfi_b32 / v_pk_mad_u16
  uint32_t sbcv = pa.h_sbc, kdv = pa.h_kd, k0v = pa.h_k0, one1 = 0x00010001u;
  uint32_t hmLo = TWO ? 0xFFFFFFFFu : 0x0000FFFFu, hmHi = 0xFFFF0000u, zero = 0u;
  asm volatile("" : "+v"(fsv), "+v"(fpv), "+v"(sbcv), "+v"(kdv), "+v"(k0v), "+v"(one1));
  asm volatile("" : "+v"(hmLo), "+v"(hmHi), "+v"(zero));
  // a[i] of this lane at step t is sA2[(t-w) mod P + ZT - M lane - i]
  const uint32_t a_lane = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)sA2 +
                          4u * (uint32_t)(ZT - M * lane - (M - 1));

  // this lane's record slots: read from the wave above, written for the one
  // below (LDS pointers, so the slot offsets fold into the ds instructions)
  // (wave 0 reads the ring rows prefetched into xr0, slot by slot)
  uint8_t *rd_wave = w > 0 ? xr + (w - 1) * HNSL * SLOT_BYTES : xr0;
  const lds_u8 *rd_base = to_lds(rd_wave + lane * REC_BYTES);
  lds_u8 *wr_base = to_lds(xr + w * HNSL * SLOT_BYTES + lane * REC_BYTES);
  // RP: a reader takes {Iyz, best} of the row above from the record of position
  // k - 1 by the address of its LDS read, not from its own record through a DPP
  // shift. rd_prev: the record of the previous position's last register, lane -
  // 1's (lane 63's for lane 0), where a lane reads register 0's {Iyz, best}.
  // The same instantiations (the flagship's) have waves 1 and 2 issue wave 0's
  // ring fetches, store the ring rows in the saddr form and inject the B code
  // from its SGPR: RP names them all.
  constexpr bool RP = VS && M == 2 && !TWO && HSK == 2;
  const lds_u8 *rd_prev = to_lds(rd_wave + ((lane + 63) & 63) * REC_BYTES);
  // V-space: all held in VGPRs (left alone, the compiler keeps the wave's part
  // in an SGPR and adds the lane's part again in every four-step group)
  if constexpr (VS) asm volatile("" : "+v"(rd_base), "+v"(wr_base));
  if constexpr (RP) asm volatile("" : "+v"(rd_prev));
  uint32_t own = (uint32_t)lane * REC_BYTES;  // the lane's record in a ring row
  const int32_t nunit = TWO ? (n + 1) / 2 : n;  // workgroup units: triples, or pairs
  for (int unit = blockIdx.x; unit < nunit; unit += gridDim.x) {
    const int tri = TWO ? 2 * unit : unit;
    const int64_t o0 = offs[3 * (int64_t)tri], o1 = offs[3 * (int64_t)tri + 1];
    const int64_t o2 = offs[3 * (int64_t)tri + 2], o3 = offs[3 * (int64_t)tri + 3];
    const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
    // TWO: the high halves score triple tri+1 (or repeat tri when n is odd)
    const bool has1 = TWO && tri + 1 < n;
    const int64_t *of1 = offs + 3 * (int64_t)(has1 ? tri + 1 : tri);
    const int64_t q0 = of1[0], q1 = of1[1], q2 = of1[2];
    const int32_t la1 = TWO ? (int32_t)(q1 - q0) : la, lb1 = TWO ? (int32_t)(q2 - q1) : lb;
    const int32_t lc1 = TWO ? (int32_t)(of1[3] - q2) : lc;
    const int32_t lbm = max(lb, lb1);
    uint8_t *ring = ring_base + (int64_t)blockIdx.x * ring_stride;

    // ---- stage A codes (padded to P, halves k/k+64M or, TWO, the two triples) and
    // B; face records in the ring
    auto a_entry = [&](int j) -> uint32_t {  // periodic in j: the pad repeats P
      const int x0 = ((j - ZT) % P + P) % P, x1 = TWO ? x0 : ((j - ZT - 64 * M) % P + P) % P;
      const uint32_t c0 = x0 < la ? SYMC << tsa_sym(seqs, o0 + x0, pa.packed) : 0u;
      const uint32_t c1 = x1 < la1 ? SYMC << tsa_sym(seqs, (TWO ? q0 : o0) + x1, pa.packed) : 0u;
      return c0 | (c1 << 16);
    };
    for (int j = threadIdx.x; j < P + ZT + A_PAD; j += 64 * NW) {
      sA2[j] = a_entry(j);
      if constexpr (A_B64) sA2s[j] = a_entry(j + 1);
    }
    for (int i = threadIdx.x; i < lbm; i += 64 * NW) {
      if constexpr (TWO)
        sB[i] = (i < lb ? SYMC << tsa_sym(seqs, o1 + i, pa.packed) : 0u) |
                ((i < lb1 ? SYMC << tsa_sym(seqs, q1 + i, pa.packed) : 0u) << 16);
      else
        sB[i] = (SYMC << tsa_sym(seqs, o1 + i, pa.packed)) * 0x00010001u;
    }
    // ring rows of wave 0's lap 0 -> ring row (t - lag) mod R at step t
    const int32_t lag = P - HSK * (NW - 1);
    // FIRSTLAP: wave 0 builds the face records of its steps [0, t_sw) from its own
    // H registers (first-lap role, ROLE 3 in step) and fetches the ring from step
    // t_sw on, a whole group at least PD steps before the last wave's first row
    // (step lag). Only the rows of steps [t_sw, lag) are filled here: every
    // other row wave 0 fetches was written by the last wave of this unit, so a
    // workspace may hold anything (an earlier unit's or launch's rows) at entry
    constexpr bool FIRSTLAP = VS;
    const int32_t t_sw = FIRSTLAP ? max(lag - PD, 0) & ~3 : 0;
    // The RP forms share wave 0's ring fetches: waves 1 and 2 issue them. (M = 2:
    // P >= 256, so lag >= 242 and t_sw >= 2 PD: the issuers' first groups exist)
    static_assert(!RP || (PD == 8 && NW >= 4), "shared fetches: two issuers, eight slots");
    if constexpr (FIRSTLAP) {
      // row 0's face cells as wave 0 meets them at step tr: x + z = tr + 2 for
      // every position ({Iy, Ixy, Iyz, best} = lam q - lam, lam q x 3); step tr
      // < lag reads ring row (tr - lag) mod R = R - lag + tr
      const int32_t n16 = (lag - t_sw) * M * 64;
      for (int32_t i = threadIdx.x; i < n16; i += 64 * NW) {
        const int32_t tr = t_sw + i / (M * 64);
        const uint32_t f1 = h_bits(pa.lam * (tr + 1)), f2 = h_bits(pa.lam * (tr + 2));
        ((uint4 *)ring)[(int64_t)(R - lag + tr) * (M * 64) + i % (M * 64)] = make_uint4(f1, f2, f2, f2);
      }
    } else {  // the message forms: every row holds the constant y = 0 face
      const uint4 face = make_uint4(pa.f_single, pa.f_pair, pa.f_pair, 0u);
      const int64_t n16 = (int64_t)R * M * 64;
      for (int64_t i = threadIdx.x; i < n16; i += 64 * NW) ((uint4 *)ring)[i] = face;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- per-position registers (arrays [2] alternate roles between even/odd steps)
    uint32_t b[M], c[M], SBC[M], K[M], DMC[M], DMB[M];
    uint32_t oIx[M], shIz[M], svIxy[M], svIyz[M], shIxz[2][M], svM[2][M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const int k0 = M * lane + i, k1 = TWO ? k0 : 64 * M + M * lane + i;
      const uint32_t c0 = k0 < lc ? SYMC << tsa_sym(seqs, o2 + k0, pa.packed) : 0u;
      const uint32_t c1 = k1 < lc1 ? SYMC << tsa_sym(seqs, (TWO ? q2 : o2) + k1, pa.packed) : 0u;
      c[i] = c0 | (c1 << 16);
      DMC[i] = w_over_code(pa.dmf, pa.dm8, c[i]);
      b[i] = SBC[i] = K[i] = DMB[i] = 0;  // set when a position reaches x = 1 of its lap
      oIx[i] = pa.f_single;
      shIz[i] = pa.f_single;
      shIxz[0][i] = shIxz[1][i] = pa.f_pair;
      svIxy[i] = svIyz[i] = pa.f_pair;
      svM[0][i] = svM[1][i] = VI ? pa.i_bias : 0u;  // (VI: f_single, f_pair are the bias too)
    }
    // END: the running key of each position (ek.v[h][i]: half h of register i)
    EndKeys<M, END> ek;
    if constexpr (END) {
#pragma unroll
      for (int i = 0; i < M; ++i) ek.v[0][i] = ek.v[1][i] = 0u;
      ek.kl = (uint32_t)(M * lane);
    }
    // position-0 bookkeeping (wave-uniform): u0 = t - w
    int32_t xpos0 = (P - ((HSK * w) % P)) % P;  // (t - HSK w) mod P at t = 0
    int32_t lap0 = w == 0 ? 0 : -1;     // floor((t - w) / P)
    // bfi half mask of the x = 1 position xpos0 -- low half below 64M, high
    // half below KS, none from KS up to the lap wrap (P > KS) -- switched at
    // those events (one compare per step) rather than tested every step
    auto hm_of = [&](int32_t xp) -> uint32_t {
      return xp >= KS ? zero : xp >= 64 * M ? hmHi : hmLo;
    };
    auto ev_of = [&](int32_t xp) -> int32_t { return xp < 64 * M ? 64 * M : xp < KS ? KS : P; };
    uint32_t hmCur = hm_of(xpos0);
    int32_t next_ev = ev_of(xpos0);
    // B code of row lap0*NW+w+1, taken by the position at x = 1 (0 past LB)
    auto b_of_lap = [&](int32_t lp) -> uint32_t {
      const int32_t r = lp * NW + w;
      return (lp >= 0 && r < lbm) ? sB[r] : 0u;
    };
    uint32_t binj = b_of_lap(lap0);
    // the per-row terms of the row whose B code is binj, for every position:
    // a position copies them when it reaches x = 1 (recomputed once per lap)
    uint32_t SBCn[M], Kn[M], DMBn = 0;
    auto row_terms = [&]() {
      if constexpr (F16) {
        // V-space: the [a=b] terms multiply the symbol code itself (a & b, no
        // min): DMB = dm / code(b) and, RTL, K = (d0 + [b=c] d1) / code(b)
        uint32_t kb0 = k0v, kbd = kdv;
        if constexpr (VS) {
          DMBn = w_over_code(pa.dmf, pa.dm8, binj);
          if constexpr (!SOP) {
            kb0 = w_over_code(pa.d0f, pa.d0_8, binj);
            const uint32_t kb1 = w_over_code(pa.d0f + pa.d1f, pa.d0_8 + pa.d1_8, binj);
            kbd = (((kb1 & 0xFFFFu) - (kb0 & 0xFFFFu)) & 0xFFFFu) | ((((kb1 >> 16) - (kb0 >> 16)) & 0xFFFFu) << 16);
          }
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {
          const uint32_t e01 = pk_eq1(binj, c[i], one1);
          SBCn[i] = pk_mad(e01, sbcv, 0u);
          Kn[i] = pk_mad(e01, kbd, kb0);
          if constexpr (VI) {  // what a 32-bit add adds: the words of the signed halves
            SBCn[i] = pk_signed(SBCn[i]);
            if constexpr (SOP) Kn[i] = pk_signed(Kn[i]);
          }
        }
      }
    };
    row_terms();
    const int32_t lap_f = (lb - 1) / NW, w_f = (lb - 1) % NW, k_f = lc - 1;
    const int32_t t_f = lap_f * P + (la - 1) + HSK * w_f + k_f;  // final cell (la, lb, lc)
    // TWO: the high-half triple's final cell, captured by its own step test
    const int32_t w_f1 = (lb1 - 1) % NW, k_f1 = lc1 - 1;
    const int32_t t_f1 = ((lb1 - 1) / NW) * P + (la1 - 1) + HSK * w_f1 + k_f1;
    const int32_t T = (TWO ? max(t_f, t_f1) : t_f) + 1;

    // VS: Hr[s & 3] = H(s) = lam * (y + xpos0) at step s (y: position 0's row,
    // 1-based) -- the x = 0 face at the x = 1 position and, one and two steps
    // ahead, the z = 0 face of position 0; step s sets H(s + 2): one v_pk_add (VI:
    // a scalar add), reset at a wrap
    uint32_t Hr[4] = {0u, 0u, 0u, 0u};
    auto hq_at = [&](int32_t s) -> int32_t {
      const int32_t u = s - HSK * w;
      const int32_t lp = u >= 0 ? u / P : -((P - 1 - u) / P);
      return pa.lam * (lp * NW + w + 1 + (u - lp * P));
    };
    if constexpr (VS) {
      // the step-0 injection's (0, y-1, z-1) face is H(0) - lam (wave 0 starts
      // its first row at step 0 with no wrap that would have set it)
      Hr[0] = h_bits(hq_at(0));
      Hr[1] = h_bits(hq_at(1));
      if constexpr (VI) Hr[3] = Hr[0] - pa.i_lam;
      else Hr[3] = U(H(Hr[0]) - H(pa.v_lam));
      if (w == 0) {  // position 0's z = 0 faces at steps 0 and 1 (as if shifted in at steps -1, -2)
#pragma unroll
        for (int i = 0; i < M; ++i) {
          shIz[i] = svIyz[i] = svM[1][i] = Hr[0];
          shIxz[1][i] = Hr[1];
        }
      }
    }
    // wave 0: prime the LDS-DMA pipeline with the rows of steps t0 .. t0 + PD - 1
    // (ring row of step s = s - lag) before its first fetching step t0 (VS: t_sw)
    int32_t dma_row = 0;  // ring row for step t + PD
    auto prime = [&](int32_t t0) {
#pragma unroll 1
      for (int s = t0; s < t0 + PD; ++s) {
        const int32_t row = ((s - lag) % R + R) % R;
#pragma unroll
        for (int i = 0; i < M; ++i)
          dma16(ring + ((int64_t)row * M + i) * PAIR_BYTES + lane * REC_BYTES,
                xr0 + (s % PD) * SLOT_BYTES + i * PAIR_BYTES);
      }
      dma_row = ((t0 + PD - lag) % R + R) % R;
    };
    if constexpr (!FIRSTLAP) {
      if (w == 0) prime(0);
    }
    // RP: issuer w (1 or 2) takes the rows of the steps = iss_j (mod 2). It issues
    // from group t_iss on, at step t the row of step t + 6 + iss_j; the first row
    // wave 0 reads is the second it issues (the very first, of step t_sw - 2 +
    // iss_j, lands in a slot nobody reads). The other waves never get there.
    const int32_t iss_j = w - 1;
    int32_t t_iss = 0x7FFFFFFF;
    if constexpr (RP) {
      if (w == 1 || w == 2) {
        t_iss = t_sw - PD;
        dma_row = ((t_iss + 6 + iss_j - lag) % R + R) % R;
      }
    }
    // byte offset of step (6 + iss_j)'s slot; step t's issue adds t slots (mod PD)
    const uint32_t iss_slot0 = (uint32_t)((6 + iss_j) * SLOT_BYTES);
    const uint32_t dvo0 = (uint32_t)lane * REC_BYTES, dvo1 = dvo0 + PAIR_BYTES;  // dma16x2_saddr's lane offsets
    const uint32_t xr0_lds = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)xr0);
    uint32_t a_nx[M];                            // A codes of the coming step (A_EVEN: the coming odd step)
    // A_EVEN: the coming even step's. An even step reads the codes of both steps
    // after it, so no LDS read is pending at the barrier that ends the odd one
    constexpr bool A_EVEN = VS;
    uint32_t a_ev[M];
    if constexpr (A_EVEN) load_a<M>(a_lane + 4u * (uint32_t)xpos0, a_ev);
    else load_a<M>(a_lane + 4u * (uint32_t)xpos0, a_nx);
    int32_t st_row = 0;                          // ring row written at step t (last wave)
    uint32_t abase = a_lane;                     // VS: A address of the group's first step
    // A_B64: the same entry in the shifted copy
    const uint32_t a_lane_s = a_lane + (uint32_t)((uint8_t *)sA2s - (uint8_t *)sA2);
    uint32_t abase_s = a_lane_s;
    const lds_u8 *r0_own = rd_base, *r0_prev = rd_prev;  // RP, wave 0: the group's four xr0 slots

    // VS: the step whose cell is the final one, in this wave (-1: none)
    const int32_t t_fin = w == w_f ? T - 1 : -1;
    // the x = 1 mask kept from the even step of a pair (step, MASK_PAIRS)
    constexpr bool MASK_PAIRS = VS && M == 2 && HSK == 2;
    uint32_t m1_pair = 0u;
    // Called by no instantiation, and kept for the compiler's sake alone. The step
    // names this lambda once, in a branch no phase takes, where it used to name
    // the retired table fetch of the face values. Without that capture every
    // kernel still gets the same instructions, but in the 19 f16-class ones the
    // two to five register copies of binj / SBCn / Kn ahead of the step loop come
    // out in another order; with it each kernel's code is byte for byte what it
    // was with the build switches. Take both lines out with the next change that
    // moves the kernel's code anyway.
    auto copy_order = [&](auto z) { return pa.lam + lane + decltype(z)::value; };
    // One step; PH = t & 1 picks the register roles and the LDS record slots,
    // ROLE the wave's place in the lap (0: wave 0, reads the ring; 3: wave 0 in
    // its first lap, before step t_sw; 2: the last wave, writes the ring; 1: the
    // others), so the loop body has no role branches.
    auto step = [&](auto ph, auto role, int32_t t, auto fin_step) {
      // ph = t & 3 (or -1: slot phase at run time); PH = t & 1 picks the registers
      constexpr int PQ = decltype(ph)::value;
      constexpr int PH = PQ & 1;
      const int32_t q = PQ >= 0 && PQ < 4 ? PQ : (t & 3);  // record slot phase
      constexpr int ROLE = decltype(role)::value & 3;
      // M = 2 with even P: the x = 1 position's register (t - w) mod 2 is
      // PH ^ (w & 1), a compile-time constant for a wave of known parity
      constexpr int WPAR = ((decltype(role)::value >> 2) & 3) - 1;  // -1: unknown
      constexpr int ISC = (M == 2 && WPAR >= 0) ? (HSK == 2 ? PH : PH ^ WPAR) : -1;
      constexpr bool FIN = decltype(fin_step)::value;  // the last step (t == T-1)
      // RP: this wave issues ring rows in this loop (role bit 5): at the even
      // steps; the odd step after waits for the oldest row before its barrier
      constexpr bool ISS = RP && ((decltype(role)::value >> 5) & 1);
      constexpr bool ISS_AT = ISS && PQ >= 0 && PQ < 4 && (PQ & 1) == 0;
      constexpr bool ISS_WAIT = ISS && PQ >= 0 && PQ < 4 && (PQ & 1) == 1;
      // this step's A codes (LDS table) and the B code of position x = 1
      uint32_t a[M];
#pragma unroll
      for (int i = 0; i < M; ++i) a[i] = (A_EVEN && PH == 0) ? a_ev[i] : a_nx[i];
      if constexpr (PQ == 99) copy_order(ph);  // no phase is 99: see copy_order
      // ---- receive the wave-above record of step t-1
      // RP: {Iy, Ixy} of the lane's own record, {Iyz, best} of position k - 1's
      // (rec[i].z / .w then hold the values already shifted, but for lane 0's
      // fix). Register 0 of the own record comes whole: its {Iyz, best} are
      // register 1's; register 0's are lane - 1's register M - 1
      uint4 rec[M];
      [[maybe_unused]] auto read_prev = [&](const lds_u8 *own_b, const lds_u8 *prev_b, int off) {
        static_assert(!RP || M == 2, "reads at position k - 1: the M = 2 helix");
        const uint4 r0 = lds_read16_at(own_b, off);
        const uint2 r1 = lds_read8_at(own_b, off + PAIR_BYTES);
        const uint2 rp = lds_read8_at(prev_b, off + (M - 1) * PAIR_BYTES + 8);
        rec[0] = make_uint4(r0.x, r0.y, rp.x, rp.y);
        rec[M - 1] = make_uint4(r1.x, r1.y, r0.z, r0.w);
      };
      if constexpr (ROLE == 0 && RP) {
        // the slot of step t is (t % PD): r0_own / r0_prev hold the group's part
        // (PD = 8, two groups), the step's is a constant offset
        static_assert(!RP || PD == 8, "reads at position k - 1: wave 0's slots as two groups of four");
        // (no vmcnt wait: the issuer waited for the row before the barrier this step follows)
        read_prev(r0_own, r0_prev, (PQ & 3) * SLOT_BYTES);
      } else if constexpr (ROLE == 0) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(M * (PD - 1)) : "memory");
        const uint8_t *src = xr0 + (t % PD) * SLOT_BYTES + lane * REC_BYTES;
#pragma unroll
        for (int i = 0; i < M; ++i) rec[i] = lds_read16(src + i * PAIR_BYTES);
      } else if constexpr (ROLE == 3) {
        // wave 0 before step t_sw: row 0's face record, x + z = t + 2 at every
        // position -- {lam (t + 1), lam (t + 2) x 3} = {H(t), H(t + 1) x 3} of
        // this wave (y = 1, xpos0 = t: no wrap before step P > t_sw)
        static_assert(ROLE != 3 || VS, "the first-lap role reads the V-space H registers");
#pragma unroll
        for (int i = 0; i < M; ++i)
          rec[i] = make_uint4(Hr[PQ & 3], Hr[(PQ + 1) & 3], Hr[(PQ + 1) & 3], Hr[(PQ + 1) & 3]);
      } else {
        const int off = (HSK == 2 ? (q + 2) & 3 : PH ^ 1) * SLOT_BYTES;
        if constexpr (RP) {
          read_prev(rd_base, rd_prev, off);
        } else {
#pragma unroll
          for (int i = 0; i < M; ++i) rec[i] = lds_read16_at(rd_base, off + i * PAIR_BYTES);
        }
      }
      uint32_t inIx[M], inIy[M], inIz[M], inIxy[M], inIyz[M], inIxz[M], inM[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        inIx[i] = oIx[i];
        inIy[i] = rec[i].x;
        inIz[i] = shIz[i];
        inIxy[i] = svIxy[i];
        inIyz[i] = svIyz[i];
        inIxz[i] = shIxz[PH][i];
        inM[i] = svM[PH][i];
      }
      // ---- x == 1 at position k* = (t - w) mod P: its x-1 inputs are the x = 0
      // face (EN_i==1&&EN==0 gating, src/PE_1cyc.v:164-178,196-202,212-218), and
      // it starts row lap0*NW+w+1, whose B symbol it takes here.
      {  // (hmCur is 0 past KS: nothing is selected there)
        int32_t ls, is, hs;
        pos_split<M>(xpos0, ls, is, hs);
        uint32_t m1;
        // M = 2, skew 2: xpos0 has t's parity, so the odd step of a pair
        // injects the same lane and half as the even one (register 1 after
        // register 0; the half-mask events and the lap wrap fall on even
        // xpos0, between pairs): its mask is the even step's
        if constexpr (MASK_PAIRS && (PQ & 1)) {
          m1 = m1_pair;
        } else {
          asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(m1) : "v"(hmCur), "s"(1ull << ls));
          if constexpr (MASK_PAIRS) m1_pair = m1;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {
          if (ISC >= 0 ? i == ISC : i == is) {
            if constexpr (VS) {  // faces (0,y,z), (0,y-1,z), (0,y,z-1): lam(y+z-1); (0,y-1,z-1): one lam less
              // (VI: H is a wave-uniform integer a scalar add advances, so it
              // lives in SGPRs with no load, and the bfi reads it from there)
              if constexpr (VI) {
                inIx[i] = vbfi_s(m1, Hr[PQ & 3], inIx[i]);
                inIxy[i] = vbfi_s(m1, Hr[PQ & 3], inIxy[i]);
                inIxz[i] = vbfi_s(m1, Hr[PQ & 3], inIxz[i]);
                inM[i] = vbfi_s(m1, Hr[(PQ + 3) & 3], inM[i]);
              } else {
                inIx[i] = vbfi(m1, Hr[PQ & 3], inIx[i]);
                inIxy[i] = vbfi(m1, Hr[PQ & 3], inIxy[i]);
                inIxz[i] = vbfi(m1, Hr[PQ & 3], inIxz[i]);
                inM[i] = vbfi(m1, Hr[(PQ + 3) & 3], inM[i]);
              }
            } else {
              inIx[i] = vbfi(m1, fsv, inIx[i]);
              inIxy[i] = vbfi(m1, fpv, inIxy[i]);
              inIxz[i] = vbfi(m1, fpv, inIxz[i]);
              inM[i] = vbfi(m1, zero, inM[i]);
            }
            // (RP forms: binj is wave-uniform and lives in an SGPR; the bfi reads it there)
            if constexpr (RP) b[i] = vbfi_s(m1, binj, b[i]);
            else b[i] = vbfi(m1, binj, b[i]);
            if constexpr (F16) {  // the new row's per-row terms (row_terms)
              SBC[i] = vbfi(m1, SBCn[i], SBC[i]);
              K[i] = vbfi(m1, Kn[i], K[i]);
              if constexpr (VS) DMB[i] = vbfi(m1, DMBn, DMB[i]);
            }
          }
        }
      }
      // keep the per-row registers in place across the branches above (without
      // this the allocator copies b into a fresh pair every step)
#pragma unroll
      for (int i = 0; i < M; ++i) asm volatile("" : "+v"(b[i]), "+v"(SBC[i]), "+v"(K[i]), "+v"(DMB[i]));
      uint32_t oIy[M], oIxy[M], oIyz[M], oBest[M], oIz[M], oIxz[M], nIx[M];
      // Priority 0 for the cell arithmetic, 1 for the send/shift/barrier tail:
      // VALU issue goes by priority then age, so without this the oldest waves
      // of a SIMD finish each step first and idle at the barrier (+3-4 %).
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);  // keep the arithmetic between the two
      if constexpr (VI)
        cell_messages_vi<M, SOP>(a, b, c, SBC, K, DMC, DMB, pv, inIx, inIy, inIz, inIxy, inIyz, inIxz, inM, nIx,
                                 oIy, oIz, oIxy, oIyz, oIxz, oBest);
      else if constexpr (VS)
        cell_messages_vs<M, SOP>(a, b, c, SBC, K, DMC, DMB, pv, inIx, inIy, inIz, inIxy, inIyz, inIxz, inM, nIx,
                                 oIy, oIz, oIxy, oIyz, oIxz, oBest);
      else if constexpr (F16)
        cell_messages_f16<M, SOP>(a, b, c, SBC, K, DMC, ones, pv, inIx, inIy, inIz, inIxy, inIyz, inIxz, inM, nIx,
                             oIy, oIz, oIxy, oIyz, oIxz, oBest);
      else
        cell_messages<M, SOP ? 1 : 0>(a, b, c, ones, pv, inIx, inIy, inIz, inIxy, inIyz, inIxz,
                                      inM, nIx, oIy, oIz, oIxy, oIyz, oIxz, oBest);

      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      // ---- the final cell (src/TriAlign_1cyc.v:141-142,342-345) is in wave w_f's
      // last step; it is read back after the loop
      if constexpr (END) {  // no corner capture: the keys are folded after the record is sent
      } else if constexpr (TWO) {  // two final cells, possibly at different steps
        if (t == t_f && w == w_f) fin[lane] = oBest[0];
        if (t == t_f1 && w == w_f1) fin[64 + lane] = oBest[0];
      } else if constexpr (VS) {  // the four-step loop runs past T: the final step is tested
        if (t == t_fin) {  // (peeling the last group instead trips a gfx950 backend bug)
#pragma unroll
          for (int i = 0; i < M; ++i) fin[i * 64 + lane] = oBest[i];
        }
      } else if constexpr (FIN) {
        if (w == w_f) {
#pragma unroll
          for (int i = 0; i < M; ++i) fin[i * 64 + lane] = oBest[i];
        }
      }

      // ---- send this step's record to the wave below (or the ring)
      if constexpr (ROLE != 2) {
        const int off = (HSK == 2 ? q : PH) * SLOT_BYTES;
#pragma unroll
        for (int i = 0; i < M; ++i)
          lds_write16_at(wr_base, off + i * PAIR_BYTES, make_uint4(oIy[i], oIxy[i], oIyz[i], oBest[i]));
      } else {
        // Positions that have not started (u = t - w - k < 0) must publish the
        // y = 0 face: wave 0 reads this row as "row y0-1" during its lap 0.
        if (t < ZT + HSK * NW) {
          const int32_t lim = t - HSK * w;  // position k started iff k <= lim
          // VS: wave 0 meets this row at step t + lag, where x + z = t + lag + 2
          const uint32_t fy = VS ? h_bits(pa.lam * (t + lag + 1)) : pa.f_single;
          const uint32_t fp = VS ? h_bits(pa.lam * (t + lag + 2)) : pa.f_pair;
          const uint32_t fb = VS ? fp : 0u;
#pragma unroll
          for (int i = 0; i < M; ++i) {
            const uint32_t m = ((M * lane + i > lim) ? 0x0000FFFFu : 0u) |
                               (((TWO ? 0 : 64 * M) + M * lane + i > lim) ? 0xFFFF0000u : 0u);
            oIy[i] = bfi(m, fy, oIy[i]);
            oIxy[i] = bfi(m, fp, oIxy[i]);
            oIyz[i] = bfi(m, fp, oIyz[i]);
            oBest[i] = bfi(m, fb, oBest[i]);
          }
        }
        // RP: a uniform row base plus the lane's unsigned 32-bit offset, which the
        // compiler selects as the store's saddr form, no 64-bit VALU address per
        // step (the offset is named in the step, or its 64-bit extension is
        // hoisted out of the loop and the add of the row base comes back)
        if constexpr (RP) asm volatile("" : "+v"(own));
        uint4 *dst = (uint4 *)__builtin_assume_aligned(
            RP ? (ring + (int64_t)st_row * SLOT_BYTES) + own : ring + (int64_t)st_row * SLOT_BYTES + lane * REC_BYTES,
            16);
#pragma unroll
        for (int i = 0; i < M; ++i) dst[i * 64] = make_uint4(oIy[i], oIxy[i], oIyz[i], oBest[i]);
      }
      // ---- END: fold this step's real cells into the positions' keys. Position k
      // holds x - 1 = xpos0 - k of row lap0 NW + w + 1 once it has wrapped
      // (k <= xpos0: class A) and x - 1 = xpos0 + P - k of the row NW above
      // otherwise (class B); each class's terms are wave-uniform (end_class).
      // The last wave's unstarted positions were overwritten above: not real.
      if constexpr (END) {
        const EndClass eA = end_class<VI>(pa, xpos0, lap0, lap0 * NW + w, la, lb);
        const EndClass eB = end_class<VI>(pa, xpos0 + P, lap0 - 1, (lap0 - 1) * NW + w, la, lb);
        if (pa.end_face) {
#pragma unroll
          for (int i = 0; i < M; ++i)
            end_fold<M, VI, true>(oBest[i], ek.kl + i, (uint32_t)(lc - 1), eA, eB, ek.v[0][i], ek.v[1][i]);
        } else {
#pragma unroll
          for (int i = 0; i < M; ++i)
            end_fold<M, VI, false>(oBest[i], ek.kl + i, (uint32_t)(lc - 1), eA, eB, ek.v[0][i], ek.v[1][i]);
        }
      }
      // ---- advance the systolic registers
#pragma unroll
      for (int i = 0; i < M; ++i) {
        oIx[i] = nIx[i];
        svIxy[i] = rec[i].y;
      }
      uint32_t rz[M], rw[M];
#pragma unroll
      for (int i = 0; i < M; ++i) { rz[i] = rec[i].z; rw[i] = rec[i].w; }
      // position 0 advances to u0 + 1
      // (V-space M = 2, P a multiple of 4: the events fall on step (2w - 1) mod 4 of a group only)
      constexpr bool EV_SKIP = VS && M == 2 && HSK == 2 && WPAR >= 0 && PQ >= 0 && PQ < 4 &&
                               (PQ & 3) != (WPAR == 0 ? 3 : 1);
      auto advance = [&]() {
        if constexpr (EV_SKIP) {
          ++xpos0;
          return;
        }
        if (__builtin_expect(++xpos0 == next_ev, 0)) {
          if (xpos0 == P) {
            xpos0 = 0;
            binj = b_of_lap(++lap0);
            row_terms();
            if constexpr (VS) {  // a new row at position 0: H(t .. t+2) restart
              const int32_t y = lap0 * NW + w + 1;
              Hr[PQ & 3] = h_bits(pa.lam * (y - 1));
              Hr[(PQ + 1) & 3] = h_bits(pa.lam * y);
              Hr[(PQ + 2) & 3] = h_bits(pa.lam * (y + 1));
            }
          }
          hmCur = hm_of(xpos0);
          next_ev = ev_of(xpos0);
        }
      };
      if constexpr (VS) {
        if constexpr (VI) {
          Hr[(PQ + 2) & 3] = Hr[(PQ + 1) & 3] + pa.i_lam;
        } else {
          Hr[(PQ + 2) & 3] = U(H(Hr[(PQ + 1) & 3]) + H(pa.v_lam));
        }
        advance();
        // z = 0 faces of position 0: (x, y, 0) and (x, y-1, 0) at step t+1,
        // (x-1, y, 0) and (x-1, y-1, 0) at step t+2
        zshift<M>(shIxz[PH], oIxz, sel, Hr[(PQ + 2) & 3]);
        zshift<M>(shIz, oIz, sel, Hr[(PQ + 1) & 3]);
        if constexpr (RP && ROLE == 3) {  // every position holds the face itself, H(t + 1)
#pragma unroll
          for (int i = 0; i < M; ++i) {
            svIyz[i] = rz[i];
            svM[PH][i] = rw[i];
          }
        } else if constexpr (RP) {  // read at position k - 1: lane 0's halves alone
          zfix<M>(svIyz, rz, sel, Hr[(PQ + 1) & 3]);
          zfix<M>(svM[PH], rw, sel, Hr[(PQ + 1) & 3]);
        } else {
          zshift<M>(svIyz, rz, sel, Hr[(PQ + 1) & 3]);
          zshift<M>(svM[PH], rw, sel, Hr[(PQ + 1) & 3]);
        }
      } else {
        zshift<M>(shIxz[PH], oIxz, sel, pa.f_pair);  // z = 0 face for position 0
        zshift<M>(shIz, oIz, sel, pa.f_single);
        zshift<M>(svIyz, rz, sel, pa.f_pair);
        zshift<M>(svM[PH], rw, sel, 0u);
        advance();
      }
      if constexpr (VS && !A_EVEN) {  // x' of step t + 1
        if constexpr (A_B64) load_a_pair<(PQ & 3) + 1>(abase, abase_s, a_nx);
        else load_a_off<M>(abase, (PQ & 3) + 1, a_nx);
      } else if constexpr (VS) {
        // x' of steps t + 1 and t + 2, both read in the even step: the odd step
        // ends at the barrier, which then waits for its record writes alone
        if constexpr (PH == 0) {
          if constexpr (A_B64) {
            load_a_pair<(PQ & 3) + 1>(abase, abase_s, a_nx);
            load_a_pair<(PQ & 3) + 2>(abase, abase_s, a_ev);
          } else {
            load_a_off<M>(abase, (PQ & 3) + 1, a_nx);
            load_a_off<M>(abase, (PQ & 3) + 2, a_ev);
          }
        }
      } else {
        load_a<M>(a_lane + 4u * (uint32_t)xpos0, a_nx);
      }

      // ---- wave 0: fetch the record of step t + PD into the slot just consumed
      if constexpr (ISS_AT) {  // the row of step t + 6 + iss_j, into that step's slot
        const uint32_t slot = ((uint32_t)t * SLOT_BYTES + iss_slot0) & (uint32_t)(PD * SLOT_BYTES - 1);
        dma16x2_saddr(ring + (int64_t)dma_row * SLOT_BYTES, dvo0, dvo1, xr0_lds + slot, xr0_lds + slot + PAIR_BYTES);
        dma_row += 2;
        if (dma_row >= R) dma_row -= R;
      }
      // the two rows issued after the one now due stay in flight (M loads a row)
      if constexpr (ISS_WAIT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * M) : "memory");
      if constexpr (ROLE == 0 && !RP) {
#pragma unroll
        for (int i = 0; i < M; ++i)
          if constexpr (M == 2) {  // the row's two pieces in one statement
            if (i == 0)
              dma16x2_saddr(ring + (int64_t)dma_row * SLOT_BYTES, dvo0, dvo1,
                            xr0_lds + (uint32_t)((t % PD) * SLOT_BYTES),
                            xr0_lds + (uint32_t)((t % PD) * SLOT_BYTES + PAIR_BYTES));
          } else
            dma16(ring + ((int64_t)dma_row * M + i) * PAIR_BYTES + lane * REC_BYTES,
                  xr0 + (t % PD) * SLOT_BYTES + i * PAIR_BYTES);
        if (++dma_row == R) dma_row = 0;
      }
      if constexpr (ROLE == 2) {
        if (++st_row == R) st_row = 0;
        constexpr int VMW = M * STORE_SLACK < 63 ? M * STORE_SLACK : 63;  // M stores per step; 6-bit vmcnt
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMW) : "memory");
      }
      // skew 2: a wave reads records two steps old, so one barrier per pair of steps
      if constexpr (HSK == 1 || PH == 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };

    // the last step is peeled off (it records the final cell), so the loop
    // body carries no final-step test; PH stays t & 1
    auto run = [&](auto role) {
      int32_t t = 0;
      const int32_t T1 = T - 1;
      // P0/P1: t & 1 known, the slot phase t & 3 read at run time (values 4, 5)
      constexpr std::integral_constant<int, 4> P0{};
      constexpr std::integral_constant<int, 5> P1{};
      constexpr std::integral_constant<int, 0> Q0{};
      constexpr std::integral_constant<int, 1> Q1{};
      constexpr std::integral_constant<int, 2> Q2{};
      constexpr std::integral_constant<int, 3> Q3{};
      constexpr std::false_type mid{};
      constexpr std::true_type last{};
      if constexpr (VS) {  // whole groups of four steps (H's phase is t & 3), the final cell tested
        auto group_bases = [&]() {  // the A addresses of the group's first step
          abase = a_lane + 4u * (uint32_t)xpos0;
          if constexpr (A_B64) abase_s = a_lane_s + 4u * (uint32_t)xpos0;
          if constexpr (RP && (decltype(role)::value & 3) == 0) {  // wave 0: slots (t & 4) .. + 3 (t % 4 == 0)
            r0_own = rd_base + (t & 4) * SLOT_BYTES;
            r0_prev = rd_prev + (t & 4) * SLOT_BYTES;
          }
        };
        if constexpr (FIRSTLAP && (decltype(role)::value & 3) == 0) {
          // wave 0's first lap: whole groups in the first-lap role (no fetch, no
          // vmcnt wait) up to step t_sw, then the fetch pipeline and ROLE 0
          constexpr std::integral_constant<int, decltype(role)::value | 3> first{};
#pragma unroll 1
          for (; t < t_sw && t < T; t += 4) {
            group_bases();
            TSA_INLINE_IF_WIDE(step(Q0, first, t, mid));
            TSA_INLINE_IF_WIDE(step(Q1, first, t + 1, mid));
            TSA_INLINE_IF_WIDE(step(Q2, first, t + 2, mid));
            TSA_INLINE_IF_WIDE(step(Q3, first, t + 3, mid));
          }
          if constexpr (!RP) {
            if (t < T) prime(t);
          }
        }
#pragma unroll 1
        for (; t < (RP && (decltype(role)::value & 3) == 1 ? min(t_iss, T) : T); t += 4) {
          group_bases();
          TSA_INLINE_IF_WIDE(step(Q0, role, t, mid));
          TSA_INLINE_IF_WIDE(step(Q1, role, t + 1, mid));
          TSA_INLINE_IF_WIDE(step(Q2, role, t + 2, mid));
          TSA_INLINE_IF_WIDE(step(Q3, role, t + 3, mid));
        }
        if constexpr (RP && (decltype(role)::value & 3) == 1) {
          // the issuers' groups from t_iss on: the same steps with the fetch
          // statements (a middle wave that issues nothing has left the loop above at T)
          constexpr std::integral_constant<int, decltype(role)::value | 32> issuing{};
#pragma unroll 1
          for (; t < T; t += 4) {
            group_bases();
            TSA_INLINE_IF_WIDE(step(Q0, issuing, t, mid));
            TSA_INLINE_IF_WIDE(step(Q1, issuing, t + 1, mid));
            TSA_INLINE_IF_WIDE(step(Q2, issuing, t + 2, mid));
            TSA_INLINE_IF_WIDE(step(Q3, issuing, t + 3, mid));
          }
        }
        return;
      }
#pragma unroll 1
      for (; (M <= 2 || HSK == 2) && t + 3 < T1; t += 4) {  // four steps a body where the step is small
        TSA_INLINE_IF_WIDE(step(Q0, role, t, mid));
        TSA_INLINE_IF_WIDE(step(Q1, role, t + 1, mid));
        TSA_INLINE_IF_WIDE(step(Q2, role, t + 2, mid));
        TSA_INLINE_IF_WIDE(step(Q3, role, t + 3, mid));
      }
#pragma unroll 1
      for (; t + 1 < T1; t += 2) {
        TSA_INLINE_IF_WIDE(step(P0, role, t, mid));
        TSA_INLINE_IF_WIDE(step(P1, role, t + 1, mid));
      }
      if (t < T1) {
        TSA_INLINE_IF_WIDE(step(P0, role, t, mid));
        TSA_INLINE_IF_WIDE(step(P1, role, t + 1, last));
      } else {
        TSA_INLINE_IF_WIDE(step(P0, role, t, last));
      }
    };
    // role | (w & 1) + 1 << 2 (M = 2, see ISC in step)
    constexpr int W0 = M == 2 ? 4 : 0, W1 = M == 2 ? 8 : 0;
    static_assert(NW % 2 == 0, "the last wave is odd");
    if (w == 0) TSA_INLINE_IF_WIDE(run(std::integral_constant<int, 0 + W0>{}));
    else if (w == NW - 1) TSA_INLINE_IF_WIDE(run(std::integral_constant<int, 2 + W1>{}));
    else if (W0 != 0 && (w & 1)) TSA_INLINE_IF_WIDE(run(std::integral_constant<int, 1 + W1>{}));
    else TSA_INLINE_IF_WIDE(run(std::integral_constant<int, 1 + W0>{}));
    if constexpr (END) {
      // z and the wave's row join the key here: {score | ~(x-1)} : ~y : ~z, so the
      // largest is the best score at the smallest x, then y, then z. Positions
      // past lc (padding in z) never enter. A wave reduce, then fin[2 w ..].
      uint64_t bk = 0;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int32_t k = M * lane + i + 64 * M * h;
          const uint32_t key = ek.v[h][i];
          if (k < lc && key != 0u) bk = umax64(bk, end_key64(key, (uint32_t)w, NW, (uint32_t)k));
        }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) bk = umax64(bk, (uint64_t)__shfl_xor((unsigned long long)bk, o, 64));
      if (lane == 0) {
        fin[2 * w] = (uint32_t)bk;
        fin[2 * w + 1] = (uint32_t)(bk >> 32);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (END) {
      if (threadIdx.x == 0) {
        uint64_t bk = 0;
        for (int j = 0; j < NW; ++j) bk = umax64(bk, ((uint64_t)fin[2 * j + 1] << 32) | fin[2 * j]);
        const uint32_t top = (uint32_t)(bk >> 32);  // {score + 2048 : 4095 - (x - 1)}
        scores[tri] = (int32_t)(top >> END_XBITS) - 2048;
        ends[3 * (int64_t)tri] = (int32_t)(END_XMASK - (top & END_XMASK)) + 1;
        ends[3 * (int64_t)tri + 1] = (int32_t)(0xFFFFu - (((uint32_t)bk >> 16) & 0xFFFFu));
        ends[3 * (int64_t)tri + 2] = (int32_t)(0xFFFFu - ((uint32_t)bk & 0xFFFFu));
      }
    } else if (threadIdx.x == 0) {
      auto decode = [&](uint16_t hb) -> int32_t {
        if constexpr (VI) return ((int32_t)hb - pa.bias) / 8;  // u = bias + 8 V
        return F16 ? (int32_t)(float)__builtin_bit_cast(_Float16, hb) : (int32_t)(int16_t)hb;
      };
      // VS: the final cell's value sits lam (la + lb + lc) above its score
      const int32_t sh0 = VS ? pa.lam * (la + lb + lc) : 0, sh1 = VS ? pa.lam * (la1 + lb1 + lc1) : 0;
      if constexpr (TWO) {
        scores[tri] = decode((uint16_t)(fin[k_f] & 0xFFFF)) - sh0;
        if (has1) scores[tri + 1] = decode((uint16_t)(fin[64 + k_f1] >> 16)) - sh1;
      } else {
        int32_t l_f, i_f, h_f;
        pos_split<M>(k_f, l_f, i_f, h_f);
        const uint32_t v = fin[i_f * 64 + l_f];
        scores[tri] = decode((uint16_t)(h_f ? (v >> 16) : (v & 0xFFFF))) - sh0;
      }
    }
    __syncthreads();
  }
}

static uint32_t pk16(int32_t v) { return ((uint32_t)(uint16_t)(int16_t)v) * 0x00010001u; }
static uint32_t pkh(double v) {  // both halves = f16(v); v exactly representable
  const _Float16 h = (_Float16)v;
  uint16_t bits;
  memcpy(&bits, &h, 2);
  return (uint32_t)bits * 0x00010001u;
}

PencilArgs make_args(const KParams &kp, bool f16, bool vs, int32_t vi_bias) {
  const int32_t GE = kp.pen[SIXY][SIX], GO = kp.pen[SIXY][SM];  // Ixy row: Ix = GE, M = GO
  int32_t fs = -kp.pen[SIX][0], fp = -kp.pen[SIXY][0];
  for (int s = 0; s < 7; ++s) {
    fs = std::max(fs, -kp.pen[SIX][s]);
    fp = std::max(fp, -kp.pen[SIXY][s]);
  }
  PencilArgs a;
  memset(&a, 0, sizeof(a));
  a.sop = kp.s3_mode == TSA_S3_SOP;
  a.packed = kp.packed;
  if (!f16) {
    a.E = pk16(GE);
    a.O = pk16(GO);
    a.E2 = pk16(2 * GE);
    a.OE = pk16(GO + GE);
    a.O2 = pk16(2 * GO);
    a.f_single = pk16(fs);
    a.f_pair = pk16(fp);
    a.dm = pk16(kp.match - kp.mismatch);
    a.mm = pk16(kp.mismatch);
    a.s3_d1 = pk16(kp.s3_eq - kp.s3_ab);
    a.s3_d0 = pk16(kp.s3_ab - kp.s3_ne);
    a.s3_ne = pk16(kp.s3_ne);
    return a;
  }
  const int32_t mm = kp.mismatch;
  a.E = pkh(GE - mm);
  a.O = pkh(GO - mm);
  a.E2 = pkh(2 * GE);
  a.OE = pkh(GO + GE);
  a.O2 = pkh(2 * GO);
  a.f_single = pkh(fs);
  a.f_pair = pkh(fp + mm);
  const int32_t dm = kp.match - mm, d0 = kp.s3_ab - kp.s3_ne, d1 = kp.s3_eq - kp.s3_ab;
  a.h_dm = pkh(dm * 8192.0);
  a.dmf = (float)dm;
  a.h_c3 = pkh((double)kp.s3_ne);
  a.h_sbc = pkh((double)dm);  // SBC = e01 * bits(dm), e01 in {0, 1}
  const uint32_t k0 = a.sop ? pkh(3.0 * mm) : pkh(d0 * 8192.0);
  const uint32_t k1 = a.sop ? pkh(3.0 * mm + dm) : pkh((d0 + d1) * 8192.0);
  a.h_k0 = k0;                // K = k0 + e01 * (k1 - k0), per 16-bit half
  a.h_kd = (((k1 & 0xFFFF) - (k0 & 0xFFFF)) & 0xFFFF) * 0x00010001u;
  if (vs) {  // cell_messages_vs: lam = GE = -mismatch; SOP's K takes the 3 lam of M
    a.lam = GE;
    a.v_lam = pkh(GE);
    a.v_cP = pkh(GO + mm + GE);
    a.v_dO = pkh(GO - GE);
    a.d0f = (float)d0;
    a.d1f = (float)d1;
    if (a.sop) {
      const uint32_t k0v = pkh(3.0 * mm + 3.0 * GE), k1v = pkh(3.0 * mm + dm + 3.0 * GE);
      a.h_k0 = k0v;
      a.h_kd = (((k1v & 0xFFFF) - (k0v & 0xFFFF)) & 0xFFFF) * 0x00010001u;
    }
    if (vi_bias != 0) {  // cell_messages_vi: u = bias + 8 V, everything scaled by 8
      a.bias = vi_bias;
      a.i_bias = (uint32_t)vi_bias * 0x00010001u;
      a.i_lam = (uint32_t)(8 * GE) * 0x00010001u;
      a.i_cP = (uint32_t)(8 * (GO + mm + GE)) * 0x00010001u;
      a.i_dO = (uint32_t)(8 * (GO - GE)) * 0x00010001u;
      a.dm8 = 8 * dm;
      a.d0_8 = 8 * d0;
      a.d1_8 = 8 * d1;
      a.f_single = a.f_pair = a.i_bias;  // initial register contents: an in-window pattern
      a.h_sbc = pk16(8 * dm);             // SBC = e01 * 8 dm per half (pk_signed in the kernel)
      a.h_k0 = pk16(8 * (3 * mm + 3 * GE));  // SOP's K = 8 (3 mismatch + 3 lam + dm [b=c])
      a.h_kd = pk16(8 * dm);
    }
  }
  return a;
}

// Intermediates of the factored form vs the candidate/state bound: a message
// is a candidate minus its score (|s3| <= 4 sc), the f16 form adds the
// mismatch back (<= sc) and splits the triple score (<= 6 sc); face messages
// sit <= 2 GO below zero. 8 sc + 4 pe covers all of them.
int64_t pencil_slack(int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend) {
  const int64_t sc = std::max(std::llabs(match), std::llabs(mismatch));
  const int64_t pe = std::max(std::llabs(gap_open), std::llabs(gap_extend));
  return 8 * sc + 4 * pe;
}

// Exact-f16 arithmetic applies when every value and intermediate is an integer
// in [-2048, 2048] (value bound +- pencil_slack) and the scaled deltas fit f16.
// The pencil_arith override (tsa_set_override; A/B and tests): "i16" forces
// the int16 form, "f16" the f16 form without V-space.
static bool arith_override(const char *want) {
  char e[8];
  return override_str("pencil_arith", e, sizeof e) && !strcmp(e, want);
}
static bool use_f16(const KParams &kp, const Range &r) {
  if (arith_override("i16")) return false;
  auto small = [](int64_t v) { return v >= -7 && v <= 7; };
  auto fits = [](int64_t v) { return v >= -2048 && v <= 2048; };
  const int64_t slack = pencil_slack(kp.match, kp.mismatch, kp.pen[SIXY][SM], kp.pen[SIXY][SIX]);
  return r.lo - slack >= -2048 && r.hi + slack <= 2048 &&
         small((int64_t)kp.match - kp.mismatch) && small((int64_t)kp.s3_ab - kp.s3_ne) &&
         small((int64_t)kp.s3_eq - kp.s3_ab) && small((int64_t)kp.s3_eq - kp.s3_ne) &&
         fits(kp.mismatch) && fits(kp.s3_ne) &&
         fits(3LL * kp.mismatch);
}

// The V-space f16 helix (cell_messages_vs) applies when lam = GE = -MISMATCH
// (the RTL constants: 1), the helix runs M <= 2, and the shifted values stay
// exact f16 integers: bound + lam (LA + LB + LC) + slack <= 2048.
static bool use_vs(const KParams &kp, const Range &r, int32_t max_la, int32_t max_lb, int32_t max_lc) {
  if (arith_override("i16") || arith_override("f16")) return false;
  const int32_t GE = kp.pen[SIXY][SIX], GO = kp.pen[SIXY][SM];
  if (!use_f16(kp, r) || pencil_pairs(max_lc) > 2 || GE < 1 || GE != -kp.mismatch || GO < GE) return false;
  const PencilGeom g = pencil_geom(max_la, max_lc);
  if (helix_lds(g.M, helix_nw(g.M), g.P, max_lb, true) > LDS_MAX) return false;  // the shifted A copy
  const int64_t slack = pencil_slack(kp.match, kp.mismatch, GO, GE);
  const int64_t hi = r.hi + (int64_t)GE * ((int64_t)max_la + max_lb + max_lc) + slack;
  return r.lo - slack >= -2048 && hi <= 2048 && (int64_t)GO + GE + kp.mismatch <= 2048;
}

// The integer-pattern V-space cell (cell_messages_vi), consulted only where
// use_vs holds: the bias, or 0 where the float cell stays. Restricted to the
// RP forms of the kernel (M = 2, not TWO, skew 2). Every half of a
// started position must stay inside [0x0400, 0x7BFF] (a carry out of a low half
// would reach a live high half), padding and run-on cells included. Those are
// cells too: a padding symbol's code is 0, which matches nothing, so the
// positions at x > LA (up to the lap period P), z > LC (up to 128 M) and in the
// rows y > LB a wave still starts before the final step (fewer than 2 NW of
// them) compute the DP of the triple extended to (P, LB + 2 NW, 128 M) by
// symbols that never match, with that problem's own faces lam q. value_bound
// assumes nothing about the symbols, so the extended problem's bound holds for
// them: r was proven for (max_la, max_lb, max_lc) and is linear in the shortest
// length (lower end) and in the coordinate sum (upper end), and is rescaled
// here, each end rounded outward. For LA = P and LC = 128 M (the 256^3 batch)
// only the 2 NW rows are added. The face values H = lam q (q <= the extended
// sum) lie under the upper end. Widened by pencil_slack for the - 8 CP, - 8 LAM
// and bonus intermediates, scaled by 8, the interval must fit the window.
// pencil_arith = f16vf keeps the float cell; f16vi is refused where this is 0.
// The integer cell runs wherever it is admitted.
constexpr int32_t VI_LO = 0x0400, VI_HI = 0x7BFF;
static int32_t use_vi(const KParams &kp, const Range &r, int32_t max_la, int32_t max_lb, int32_t max_lc) {
  if (arith_override("f16vf") || !use_vs(kp, r, max_la, max_lb, max_lc)) return 0;
  const PencilGeom g = pencil_geom(max_la, max_lc);
  if (g.M != 2 || g.two) return 0;
  const int32_t GE = kp.pen[SIXY][SIX], GO = kp.pen[SIXY][SM];
  const int64_t e_la = g.P, e_lb = (int64_t)max_lb + 2 * helix_nw(g.M), e_lc = 128 * g.M;
  const int64_t mn = std::min<int64_t>(max_la, std::min(max_lb, max_lc)), e_mn = std::min(e_la, std::min(e_lb, e_lc));
  const int64_t q = (int64_t)max_la + max_lb + max_lc, e_q = e_la + e_lb + e_lc;
  const int64_t lo = -((-std::min<int64_t>(r.lo, 0) * e_mn + mn - 1) / mn);  // r.lo <= 0, linear in mn
  const int64_t hi = ((std::max<int64_t>(r.hi, 0) + 1) * e_q + q - 1) / q;   // r.hi = floor(gain q)
  const int64_t slack = pencil_slack(kp.match, kp.mismatch, GO, GE);
  const int64_t v_lo = lo - slack, v_hi = hi + (int64_t)GE * e_q + slack;
  if (8 * (v_hi - v_lo) > VI_HI - VI_LO) return 0;
  return (int32_t)(VI_LO - 8 * v_lo);
}

// The lap kernel's V-space cell (lap_kernel VS) under the same conditions as
// the helix's, for any tile width: lam = GE = -MISMATCH and the shifted
// values exact f16 integers.
// Opt-in (override lap_vs=1): measured slower than the message form on MI355X
// (64^3 0.098 vs 0.087 ms, 256^3 0.412 vs 0.389 ms, same box,
// profiles/r4c_lapvs.jsonl) -- the chained lap step is bound by its loader's
// hand-off, not by the cell's instructions, and the V-space faces make lap 0's
// wave 0 wait on its loader, which the message form's constant faces do not.
static bool lap_vs_ok(const KParams &kp, const Range &r, int32_t max_la, int32_t max_lb, int32_t max_lc) {
  long on = 0;
  if (!override_int("lap_vs", &on) || on == 0) return false;
  if (arith_override("i16") || arith_override("f16")) return false;
  const int32_t GE = kp.pen[SIXY][SIX], GO = kp.pen[SIXY][SM];
  if (!use_f16(kp, r) || GE < 1 || GE != -kp.mismatch || GO < GE) return false;
  const int64_t slack = pencil_slack(kp.match, kp.mismatch, GO, GE);
  const int64_t hi = r.hi + (int64_t)GE * ((int64_t)max_la + max_lb + max_lc) + slack;
  return r.lo - slack >= -2048 && hi <= 2048 && (int64_t)GO + GE + kp.mismatch <= 2048;
}

// d_ends: the end search's instantiation (END) of the same arithmetic
template <int M, int NW, bool F16, bool SOP>
static int launch_m(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                    int32_t max_lb, const PencilGeom &g, int32_t *d_scores, void *d_ws,
                    const PencilArgs &pa, hipStream_t stream, int32_t *d_ends = nullptr) {
  constexpr bool VSOK = F16 && M <= 2;  // V-space instantiations
  const bool vs = VSOK && pa.lam != 0;
  const int32_t lds_a = 4 * (g.P + 128 * M + A_PAD), lds_b = 4 * ((max_lb + 3) & ~3);
  const size_t lds = helix_lds(M, NW, g.P, max_lb, vs);
  // TWO (two triples per workgroup) exactly when pencil_geom sized P for it
  const bool two = M == 1 && g.two;
  auto kfn = vs ? (two ? pencil_kernel<M, NW, F16, SOP, M == 1, VSOK> : pencil_kernel<M, NW, F16, SOP, false, VSOK>)
                : (two ? pencil_kernel<M, NW, F16, SOP, M == 1, false> : pencil_kernel<M, NW, F16, SOP, false, false>);
  if constexpr (VSOK && M == 2) {  // the integer-pattern cell (use_vi set the bias)
    if (vs && pa.bias != 0) kfn = pencil_kernel<M, NW, F16, SOP, false, VSOK, true>;
  }
  if (d_ends) {
    if constexpr (VSOK) {
      if (two) return TSA_EINVAL;
      kfn = vs ? pencil_kernel<M, NW, F16, SOP, false, VSOK, false, true>
               : pencil_kernel<M, NW, F16, SOP, false, false, false, true>;
      if constexpr (M == 2) {
        if (vs && pa.bias != 0) kfn = pencil_kernel<M, NW, F16, SOP, false, VSOK, true, true>;
      }
    } else {
      return TSA_ERANGE;  // no end search in the int16 form or beyond M = 2
    }
  }
  if (lds > LDS_MAX) return TSA_EINVAL;
  const int32_t units = two ? (n + 1) / 2 : n;
  const int grid = units < 65535 ? units : 65535;
  return launch_with_lds((const void *)kfn, lds, [&] {
           hipLaunchKernelGGL(kfn, dim3(grid), dim3(64 * NW), lds, stream, d_seqs, d_offsets, n, g.P, g.R, lds_a,
                              lds_b, g.ring_bytes_per_triple, (uint8_t *)d_ws, d_scores, pa, d_ends);
         }) == hipSuccess
             ? TSA_OK
             : TSA_EDEVICE;
}

void pencil_describe(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                     const Range &bound, LapPolicy lap, char *buf, size_t len, bool checked) {
  const bool f16 = checked ? false : use_f16(kp, bound);
  const char *arith = f16 ? "f16" : "i16";
  const char *s3 = kp.s3_mode == TSA_S3_SOP ? "sop" : "rtl";
  const LapGeom lg = lap_choice(n, max_la, max_lb, max_lc, lap, f16, kp.s3_mode == TSA_S3_SOP, checked);
  if (lg.ok) {
    if (f16 && lap_vs_ok(kp, bound, max_la, max_lb, max_lc)) arith = "f16v";  // the lap's V-space cell
    char chunk[32] = "";
    if (lg.chunk > 0) snprintf(chunk, sizeof chunk, " chunk=%d", lg.chunk);
    snprintf(buf, len, "pencil lap %s %s M=%d NW=%d laps=%d tiles=%d waves=%lld wpc=%d%s%s est=%.0fus", arith, s3,
             lg.M, lg.NW, lg.G, lg.GZ, (long long)lg.waves, lg.per_cu, chunk, checked ? " checked" : "", lg.est_us);
    return;
  }
  const PencilGeom g = pencil_geom(max_la, max_lc);
  if (use_vs(kp, bound, max_la, max_lb, max_lc)) arith = "f16v";  // the helix's V-space cell
  const bool vi = !checked && use_vi(kp, bound, max_la, max_lb, max_lc) != 0;  // on integer patterns
  snprintf(buf, len, "pencil helix %s %s M=%d NW=%d P=%d%s est=%.0fus", arith, s3, g.M, helix_nw(g.M), g.P,
           g.two ? " two" : vi ? " int" : "", helix_est(n, max_la, max_lb, max_lc));
}

// The end search (tsa_score_batch_ends, face and any): always the helix, one
// triple per workgroup, in f16-class arithmetic. TSA_OK when the request is
// admitted: LC <= 256, and the key's fields hold every real cell (end_fold: x - 1
// in 12 bits, the lap in 8; the score by use_f16). TSA_ERANGE otherwise;
// TSA_EINVAL for a set pencil_mode other than helix, and for pencil_arith =
// f16vi where the integer cell is not admitted (as pencil_launch_batch).
int pencil_ends_admit(int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp, const Range &bound) {
  char mode[16] = "";
  if (override_str("pencil_mode", mode, sizeof mode) && strcmp(mode, "helix")) return TSA_EINVAL;
  if (!pencil_shape_ok(max_la, max_lb, max_lc) || !use_f16(kp, bound) || pencil_pairs(max_lc) > 2)
    return TSA_ERANGE;
  if (max_la - 1 > (int32_t)END_XMASK || (max_lb - 1) / helix_nw(pencil_pairs(max_lc)) > (int32_t)END_LAPMASK)
    return TSA_ERANGE;
  const PencilGeom g = pencil_geom(max_la, max_lc, true);
  const bool vs = use_vs(kp, bound, max_la, max_lb, max_lc);
  if (helix_lds(g.M, helix_nw(g.M), g.P, max_lb, vs) > LDS_MAX) return TSA_ERANGE;
  if (arith_override("f16vi") && use_vi(kp, bound, max_la, max_lb, max_lc) == 0) return TSA_EINVAL;
  return TSA_OK;
}

size_t pencil_ends_workspace_bytes(int32_t n, int32_t max_la, int32_t max_lc) {
  return (size_t)std::min<int32_t>(n, 65535) * (size_t)pencil_geom(max_la, max_lc, true).ring_bytes_per_triple;
}

// pencil_describe's helix text with the end mode in place of the estimate
// (helix_est is the plain score's)
void pencil_describe_ends(int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp, const Range &bound,
                          bool face, char *buf, size_t len) {
  const PencilGeom g = pencil_geom(max_la, max_lc, true);
  const bool vs = use_vs(kp, bound, max_la, max_lb, max_lc);
  const bool vi = use_vi(kp, bound, max_la, max_lb, max_lc) != 0;
  snprintf(buf, len, "pencil helix %s %s M=%d NW=%d P=%d%s ends=%s", vs ? "f16v" : "f16",
           kp.s3_mode == TSA_S3_SOP ? "sop" : "rtl", g.M, helix_nw(g.M), g.P, vi ? " int" : "", face ? "face" : "any");
}

int pencil_launch_ends(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t max_la,
                       int32_t max_lb, int32_t max_lc, const KParams &kp, const Range &bound, bool face,
                       int32_t *d_scores, int32_t *d_ends, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  if (n <= 0) return TSA_OK;
  if (!d_ends) return TSA_EINVAL;
  const int rc = pencil_ends_admit(max_la, max_lb, max_lc, kp, bound);
  if (rc) return rc;
  if (n > 65535) return TSA_EINVAL;  // the callers chunk
  const bool sop = kp.s3_mode == TSA_S3_SOP;
  PencilArgs pa = make_args(kp, true, use_vs(kp, bound, max_la, max_lb, max_lc),
                            use_vi(kp, bound, max_la, max_lb, max_lc));
  pa.end_face = face ? 1 : 0;
  const PencilGeom g = pencil_geom(max_la, max_lc, true);
  if (ws_bytes < (size_t)n * (size_t)g.ring_bytes_per_triple) return TSA_ENOMEM;
  if (g.M == 1)
    return sop ? launch_m<1, 8, true, true>(d_seqs, d_offsets, n, max_lb, g, d_scores, d_ws, pa, stream, d_ends)
               : launch_m<1, 8, true, false>(d_seqs, d_offsets, n, max_lb, g, d_scores, d_ws, pa, stream, d_ends);
  return sop ? launch_m<2, 8, true, true>(d_seqs, d_offsets, n, max_lb, g, d_scores, d_ws, pa, stream, d_ends)
             : launch_m<2, 8, true, false>(d_seqs, d_offsets, n, max_lb, g, d_scores, d_ws, pa, stream, d_ends);
}

// The end search on the lap schedule (tsa_score_batch_ends_lap, face and any):
// always the checked kernel's int16 plan with the key fold (lap_ends_kernel),
// never the helix. TSA_OK when a lap plan exists for the batch among the
// instantiated geometries (M <= 2; lap_m, lap_nw and lap_chunk hold) and the
// key's 16 bits hold x - 1; TSA_ERANGE otherwise; TSA_EINVAL for a set
// pencil_mode other than lap.
static LapGeom lap_ends_choice(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                               LapPolicy lap) {
  return lap_choice(n, max_la, max_lb, max_lc, lap, false, kp.s3_mode == TSA_S3_SOP, true, true);
}
int pencil_lap_ends_admit(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                          LapPolicy lap) {
  char mode[16] = "";
  if (override_str("pencil_mode", mode, sizeof mode) && strcmp(mode, "lap")) return TSA_EINVAL;
  if (!pencil_shape_ok(max_la, max_lb, max_lc) || max_la - 1 > 0xFFFE) return TSA_ERANGE;
  return lap_ends_choice(n, max_la, max_lb, max_lc, kp, lap).ok ? TSA_OK : TSA_ERANGE;
}

size_t pencil_lap_ends_workspace_bytes(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                                       LapPolicy lap) {
  const LapGeom g = lap_ends_choice(n, max_la, max_lb, max_lc, kp, lap);
  return g.ok ? lap_ends_workspace_bytes(g) : 0;
}

// pencil_describe's checked lap text with the end mode in place of the
// estimate (lap_geom's is the plain score's); checked: certification runs
void pencil_describe_lap_ends(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                              LapPolicy lap, bool checked, bool face, char *buf, size_t len) {
  const LapGeom lg = lap_ends_choice(n, max_la, max_lb, max_lc, kp, lap);
  char chunk[32] = "";
  if (lg.chunk > 0) snprintf(chunk, sizeof chunk, " chunk=%d", lg.chunk);
  snprintf(buf, len, "pencil lap i16 %s M=%d NW=%d laps=%d tiles=%d waves=%lld wpc=%d%s%s ends=%s",
           kp.s3_mode == TSA_S3_SOP ? "sop" : "rtl", lg.M, lg.NW, lg.G, lg.GZ, (long long)lg.waves, lg.per_cu, chunk,
           checked ? " checked" : "", face ? "face" : "any");
}

int pencil_launch_lap_ends(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, int32_t max_la,
                           int32_t max_lb, int32_t max_lc, const KParams &kp, bool face, int32_t *d_scores,
                           int32_t *d_ends, void *d_ws, size_t ws_bytes, hipStream_t stream, LapPolicy lap,
                           int32_t **d_err, const CheckLimits *chk) {
  if (d_err) *d_err = nullptr;
  if (n <= 0) return TSA_OK;
  if (!d_ends) return TSA_EINVAL;
  const int rc = pencil_lap_ends_admit(n, max_la, max_lb, max_lc, kp, lap);
  if (rc) return rc;
  const LapGeom lg = lap_ends_choice(n, max_la, max_lb, max_lc, kp, lap);
  if (ws_bytes < lap_ends_workspace_bytes(lg)) return TSA_ENOMEM;
  PencilArgs pa = make_args(kp, false, false);
  pa.end_face = face ? 1 : 0;
  return lap_launch_ends(lg, kp.s3_mode == TSA_S3_SOP, d_seqs, d_offsets, n, d_scores, d_ends, d_ws, pa, stream,
                         d_err, chk);
}

int pencil_launch_batch(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                        int32_t max_la, int32_t max_lb, int32_t max_lc, const KParams &kp,
                        const Range &bound, int32_t *d_scores, void *d_ws, size_t ws_bytes,
                        hipStream_t stream, LapPolicy lap, int32_t **d_err,
                        const CheckLimits *chk) {
  if (d_err) *d_err = nullptr;
  if (n <= 0) return TSA_OK;
  if (!pencil_shape_ok(max_la, max_lb, max_lc)) return TSA_EINVAL;
  const bool f16 = chk ? false : use_f16(kp, bound);  // the checked kernel runs int16
  const bool sop = kp.s3_mode == TSA_S3_SOP;
  const LapGeom lg = lap_choice(n, max_la, max_lb, max_lc, lap, f16, sop, chk != nullptr);
  const int32_t vi_bias = chk ? 0 : use_vi(kp, bound, max_la, max_lb, max_lc);
  if (arith_override("f16vi") && (lg.ok || vi_bias == 0)) return TSA_EINVAL;  // no integer cell for this launch
  if (lg.ok) {
    if (ws_bytes < lap_workspace_bytes(lg)) return TSA_ENOMEM;
    const bool lvs = f16 && lap_vs_ok(kp, bound, max_la, max_lb, max_lc);
    return lap_launch(lg, f16, sop, d_seqs, d_offsets, n, d_scores, d_ws, make_args(kp, f16, lvs), stream,
                      d_err, chk);
  }
  const PencilArgs pa = make_args(kp, f16, !chk && use_vs(kp, bound, max_la, max_lb, max_lc), vi_bias);
  if (chk) return TSA_ERANGE;  // no lap schedule for this batch
  const PencilGeom g = pencil_geom(max_la, max_lc);
  const int32_t grid = n < 65535 ? n : 65535;
  if (ws_bytes < (size_t)grid * (size_t)g.ring_bytes_per_triple) return TSA_ENOMEM;
  return TSA_SHAPES(launch_m, g.M, f16, sop, d_seqs, d_offsets, n, max_lb, g,
                    d_scores, d_ws, pa, stream);
}

// A single cube split over np devices by laps: the lap schedule of this cube
// (whatever the helix would cost), if it has at least np laps.
LapGeom pencil_split_geom(int32_t la, int32_t lb, int32_t lc, const KParams &kp, const Range &bound,
                          int np) {
  LapGeom g{};
  g.ok = false;
  if (np < 1 || !pencil_shape_ok(la, lb, lc)) return g;
  const bool f16 = use_f16(kp, bound), sop = kp.s3_mode == TSA_S3_SOP;
  g = lap_choice(1, la, lb, lc, LAP_RESIDENT, f16, sop, true);
  if (!g.ok || g.G < np) {
    g.ok = false;
    return g;
  }
  // full-length rings: no producer ever waits for its consumer, so a part
  // whose launch queues behind an earlier part (parts sharing a hardware
  // queue) cannot deadlock it -- the only waits point from later parts to
  // earlier ones, which are launched first
  return lap_geom(1, la, lb, lc, g.M, g.NW, true, f16, sop);
}

int pencil_launch_split(const LapGeom &g, const KParams &kp, const Range &bound, const LapPart *parts,
                        int np, int32_t *d_score, uint32_t *d_err) {
  const bool f16 = use_f16(kp, bound);
  const PencilArgs pa = make_args(kp, f16, false);
  return lap_launch_split(g, f16, pa.sop != 0, pa, parts, np, d_score, d_err);
}
#undef TSA_SHAPES
#undef TSA_ARITH

}  // namespace tsa