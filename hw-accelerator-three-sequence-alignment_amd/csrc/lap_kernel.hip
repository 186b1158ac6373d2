// lap_kernel.hip -- TSA_KERNEL_PENCIL single-cube (lap) schedule.
//
// One cube (or a few) is cut into laps of RW = 2*NW rows (y) and z-tiles of
// ZT = 64*M positions; every (lap, tile) is its own workgroup and all of them
// run at once, chained through global memory -- the reference's slicing of
// the (y,z) plane into pencils with face SRAMs between them
// (src/TriAlign_1cyc.v:78-98,127-140, pic/Memory.png), with workgroups in place
// of the 8x8 PE array's passes and HBM rings in place of the face SRAMs.
//
// Inside a workgroup (tools/lap_emu.py replays this schedule on the CPU):
//  * NW compute waves; wave w holds TWO DP rows, y = L*RW + 2w + 1 in the low
//    16-bit half and y + 1 in the high half of every packed register;
//  * lane l, register i is tile position k = M*l + i (z = q*ZT + k + 1); half
//    h of wave w computes x = t - (2w + h) - k + 1 at local step t;
//  * the high half's row above is the wave's own low half one step earlier, the
//    low half's is wave w-1's high half of step t-1: one v_alignbit/v_perm per
//    record word (REC = {above.hi, own_prev.lo});
//  * z-1 neighbours shift one position per step (register rename, one DPP
//    wave_ror + one v_perm per message), the x = 1 position takes the x = 0
//    face (src/PE_1cyc.v:164-218 EN_i gating), as in the helix kernel.
// No workgroup barrier per step: the waves are a pipeline, each running its
// own loop and synchronised point to point through LDS (a systolic array of
// waves, as the RTL's PEs are one of registers):
//  * wave w writes its record of step t into an LDS ring of K slots and then
//    its progress word (t + 1); wave w+1 polls that word before reading, and
//    wave w polls wave w+1's before reusing a slot. A step costs one wave's
//    own instruction stream; the hand-off latency is paid once per wave, not
//    once per step (a barrier makes every step pay it);
//  * wave NW is the LOADER: it LDS-DMAs the records of the lap above (y) and of
//    the tile to the left (z) LPD steps ahead, checks their tags, re-fetches
//    stale ones and publishes its own progress word, which wave 0 polls -- the
//    global hand-off's latency and checks are off the compute waves' path.
// Between workgroups (MI355X_MICROARCH.md "handoff-1to1"):
//  * the last compute wave stores its per-step record (the high halves the
//    next lap's wave 0 needs) into a y ring of YR slots, and every wave's
//    lane 63 its last position ({Iz, Ixz, REC.z, REC.w}) into a z ring of ZR
//    slots for tile q+1;
//  * every 8-byte granule of a record carries a 32-bit tag of (launch epoch,
//    step), written by one sc1 store; the loader checks the tags (no flags on
//    the fast path); a stale tag re-fetches (bounded; on timeout the launch's
//    error word is set and the triple reports TSA_SCORE_INVALID);
//  * the rings are O(N^2) (O(N) per workgroup): a consumer publishes how far
//    its loader has checked, and a producer about to overwrite a slot the
//    consumer may still need waits for it (never on the fast path: the rings
//    hold 2-4x the natural lag);
//  * block b -> XCD b % 8 (observed dispatch, speed only): every lap of a z-tile
//    lands on one XCD, so the y chain's hand-offs stay in one L2's reach.
// A consumer only waits on laps of lower index (lap-major order), and a
// producer waits (back-pressure) only on a consumer of its own round -- across
// a round boundary its ring is full length. A grid beyond the resident slots is
// launched as one resident round (8 x SX workgroups) whose workgroups loop over
// their slots' later-round laps in lap order (up to LAP_MAX_WAVES rounds, any
// workgroups per CU), so no wait depends on the dispatcher's order; forward
// progress needs every launched workgroup co-resident (every wait is bounded
// and reports TSA_SCORE_INVALID).

#include <unistd.h>

#include <atomic>
#include <ctime>
#include <mutex>
#include <vector>

#include "pencil_common.h"
#include "lap_kernel.h"
#include "kernel_meta.h"

namespace tsa {

#ifndef TSA_LAP_PD1  // loader prefetch distance (steps) by M: build-time knobs. Short
#define TSA_LAP_PD1 2  // wins: a fetch issued before its producer stored is a tag miss
#endif                 // and a serial re-fetch (A/B on MI355X: 2 < 3 < 4 < 6)
#ifndef TSA_LAP_PD2
#define TSA_LAP_PD2 2
#endif
#ifndef TSA_LAP_PD4
#define TSA_LAP_PD4 3
#endif
__host__ __device__ constexpr int lap_pd(int M) {
  return M == 1 ? TSA_LAP_PD1 : M == 2 ? TSA_LAP_PD2 : TSA_LAP_PD4;
}
// LDS ring slots: wave -> wave (K) and loader -> wave 0 (K0); powers of 2
__host__ __device__ constexpr int lap_k(int M) { return M == 1 ? 4 : 2; }
__host__ __device__ constexpr int lap_k0(int M) { return M <= 2 ? 8 : 4; }
constexpr int LAP_ZL = 32;           // z records resident in LDS (power of 2)
constexpr int LAP_PUB = 4;           // the last wave publishes the consumer progress every LAP_PUB steps
constexpr int LAP_PROG_STRIDE = 32;  // progress words 128 B apart (one line each)
constexpr int LAP_ZREC_WAVE = 32;    // z record bytes per wave: 2 x {payload, tag, payload, tag}

static_assert(LAP_ZL >= 8 + 2 + TSA_LAP_PD1 + 2 && LAP_ZL >= 8 + 2 + TSA_LAP_PD2 + 2, "z slots");

// Tag of the record of step s in the launch with epoch e (32-bit): distinct
// steps of one launch never collide (odd multiplier).
__host__ __device__ __forceinline__ uint32_t lap_tag(uint32_t e, int32_t s) {
  return e ^ ((uint32_t)s * 0x9E3779B1u);
}

// A code pairs the table holds: the LIT loader reads a few entries further
// (its z = 0 faces run ZA steps ahead of the last compute step)
__host__ __device__ constexpr int32_t lap_na(int32_t la, int M, int NW, bool lit) {
  return la + 2 * 64 * M + 4 * NW + 8 + (lit ? 2 * NW + 8 : 0);
}
// final-cell words: best of the final step, or (LIT) its 7 input states + 8
__host__ __device__ constexpr int lap_fin_words(int M, bool lit) { return lit ? 7 * M * 64 + 8 : M * 64; }
static size_t lap_lds_bytes(int M, int NW, int32_t max_la, bool lit = false) {
  const int SLOT = M * 1024;
  return (size_t)(NW - 1) * lap_k(M) * SLOT + (size_t)lap_k0(M) * SLOT +
         (size_t)LAP_ZL * NW * LAP_ZREC_WAVE + (size_t)SLOT + (size_t)NW * LAP_ZREC_WAVE + 16 * 4 +
         (size_t)(NW + 1) * 256 + (size_t)lap_fin_words(M, lit) * 4 +
         4 * (((size_t)lap_na(max_la, M, NW, lit) + 3) & ~(size_t)3);
}

// Trace slots per block (override lap_trace): 8, plus with TSA_DIAG (the
// diagnostic build, scripts/build_variant.sh) 4 shader-clock accumulators per
// compute wave and the largest producer-consumer lag (steps) seen by the y and
// z stores -- the ring slots that workgroup needed.
#if defined(TSA_DIAG)
constexpr int LAP_TRACE_SLOTS = 8 + 4 * 8 + 2;
#else
constexpr int LAP_TRACE_SLOTS = 8;
#endif

// ---------------------------------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// The s_nop: a VMEM store of more than 8 bytes must not have its data VGPRs
// rewritten by the next VALU instruction (one wait state); the compiler's
// hazard recognizer does not look inside inline asm, so the asm carries it.
// SYS (a cube split over devices, lap_launch_split): system scope (sc0 sc1),
// so a record written into a peer device's fine-grained ring is visible there.
template <bool SYS = false>
__device__ __forceinline__ void store16_sc1(void *gptr, uint4 v) {
  const u32x4 d = {v.x, v.y, v.z, v.w};
  if constexpr (SYS)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(gptr), "v"(d) : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(gptr), "v"(d) : "memory");
}
// the same store at sbase + voff + OFFB (SGPR base, 32-bit VGPR offset, immediate)
template <bool SYS, int OFFB>
__device__ __forceinline__ void store16_sc1_s(const uint8_t *sbase, uint32_t voff, uint4 v) {
  static_assert(OFFB >= 0 && OFFB < 4096, "13-bit signed global offset");
  const u32x4 d = {v.x, v.y, v.z, v.w};
  if constexpr (SYS)
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc0 sc1\n\ts_nop 1" ::"v"(voff), "v"(d), "s"(sbase),
                 "i"(OFFB)
                 : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" ::"v"(voff), "v"(d), "s"(sbase),
                 "i"(OFFB)
                 : "memory");
}
// the same store at gptr + OFFB (the instruction's immediate offset)
template <bool SYS, int OFFB>
__device__ __forceinline__ void store16_sc1_at(void *gptr, uint4 v) {
  static_assert(OFFB >= 0 && OFFB < 4096, "13-bit signed global offset");
  const u32x4 d = {v.x, v.y, v.z, v.w};
  if constexpr (SYS)
    asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc0 sc1\n\ts_nop 1" ::"v"(gptr), "v"(d), "i"(OFFB)
                 : "memory");
  else
    asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" ::"v"(gptr), "v"(d), "i"(OFFB)
                 : "memory");
}
__device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
  return __builtin_amdgcn_perm(s0, s1, sel);
}
// {above.hi -> lo, own.lo -> hi}: the row above of both halves
__device__ __forceinline__ uint32_t rows2(uint32_t own, uint32_t above) {
  return __builtin_amdgcn_alignbit(own, above, 16);
}
// f16 bits of the integer lam * v in both halves (V-space face values; exact
// below 2048 in magnitude, which the host's range check guarantees)
__device__ __forceinline__ uint32_t lam_bits(int32_t lam, int32_t v) {
  const _Float16 h = (_Float16)(float)(lam * v);
  return (uint32_t)__builtin_bit_cast(uint16_t, h) * 0x00010001u;
}
// A wave-uniform 64-bit lane mask, forced into an SGPR pair (the compiler may
// compute a uniform shift in VALU and hand the VGPR pair to an "s" operand)
__device__ __forceinline__ uint64_t sgpr64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int32_t lds_word(const int32_t *p) {
  return __builtin_amdgcn_readfirstlane(
      *(volatile const __attribute__((address_space(3))) int32_t *)(
          const __attribute__((address_space(3))) void *)p);
}
// Progress word store: every lane writes its own copy (pw[wave][lane], one
// conflict-free ds_write_b32, no exec toggling); readers read lane 0's. LDS
// executes a wave's DS instructions in order, so a reader that sees the word
// also sees the record written before it; the empty asm keeps the compiler
// from moving LDS accesses across it.
__device__ __forceinline__ void lds_publish(int32_t *pw_wave, int32_t v, int lane) {
  asm volatile("" ::: "memory");
  *(volatile __attribute__((address_space(3))) int32_t *)(__attribute__((address_space(3))) void *)(
      pw_wave + lane) = v;
  asm volatile("" ::: "memory");
}
// Lane bit `k` of a 64-bit exec-style mask when 0 <= k < 64, else 0 -- in SALU
// (left to itself the compiler shifts a 64-bit 1 in VALU and reads it back).
__device__ __forceinline__ uint64_t lane_bit(int32_t k) {
  uint64_t r;
  asm("s_lshl_b64 %0, 1, %1\n\ts_cmp_lt_u32 %1, 64\n\ts_cselect_b64 %0, %0, 0"
      : "=&s"(r) : "s"(k) : "scc");
  return r;
}

// The lap kernel's cell, split at the row above (the message form of
// cell_messages_f16 / cell_messages, src/PE_1cyc.v:159-218): of a step's
// inputs only Iy comes from this step's record -- x-1, z-1, the diagonals and
// the scores are known when the step starts -- so every message is folded to
// max(Y - c, N) with the N's computed while the record is read. GO >= GE
// orders the penalties (E <= O, 2E <= O+E <= 2O, f16 form with the mismatch
// folded into E and O alike), so Y's dominated copies drop out:
//   best = max(Y, W),       W  = max(X, Z, XY, XZ, YZ, M)
//   Ix'  = max(Y - OE, N1), N1 = max(X - 2E, U1 - OE, W - 2O), U1 = max(X, Z, XY, XZ)
//   Iy'  = max(Y - 2E, N2), N2 = max(U2 - OE, W - 2O),         U2 = max(X, Z, XY, YZ)
//   Iz'  = max(Y - OE, N3), N3 = max(Z - 2E, U3 - OE, W - 2O), U3 = max(X, Z, XZ, YZ)
//   Ixy' = max(Y - E, N4),  N4 = max(max(X, XY) - E, W - O)
//   Iyz' = max(Y - E, N5),  N5 = max(max(YZ, Z) - E, W - O)
//   Ixz' = max(Y - O, N6),  N6 = max(max(X, Z, XZ) - E, W - O)
// (11 dependent instructions per pair after the record lands instead of ~30).
template <int M>
struct LapPre {
  uint32_t W[M], N1[M], N2[M], N3[M], N4[M], N5[M], N6[M];
};
template <int M, bool SOP>
__device__ __forceinline__ void lap_pre_f16(const uint32_t (&a)[M], const uint32_t (&b)[M],
                                            const uint32_t (&c)[M], const uint32_t (&SBC)[M],
                                            const uint32_t (&K)[M], const uint32_t (&DMC)[M],
                                            uint32_t Q, const PencilArgs &pa,
                                            const uint32_t (&inIx)[M], const uint32_t (&inIz)[M],
                                            const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M],
                                            const uint32_t (&inIxz)[M], const uint32_t (&inM)[M],
                                            LapPre<M> &p) {
  const h2 DM = H(pa.h_dm), E = H(pa.E), O = H(pa.O), E2 = H(pa.E2), OE = H(pa.OE), O2 = H(pa.O2);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const h2 eab = H(umin2(a[i] & b[i], Q)), eac = H(a[i] & c[i]), DMCi = H(DMC[i]);
    const h2 sXY = hfma(eab, DM, H(inIxy[i]));  // src/PE_1cyc.v:159-161 (+mismatch folded)
    const h2 sXZ = hfma(eac, DMCi, H(inIxz[i]));
    const h2 sYZ = H(inIyz[i]) + H(SBC[i]);
    h2 sM;                                       // src/PE_1cyc.v:162
    if constexpr (SOP) sM = hfma(eab, DM, hfma(eac, DMCi, H(inM[i]))) + H(K[i]);
    else sM = hfma(eab, H(K[i]), H(inM[i])) + H(pa.h_c3);
    const h2 X = H(inIx[i]), Z = H(inIz[i]);
    const h2 pXZ = hmax(X, Z);
    const h2 U1 = vmax3(pXZ, sXY, sXZ), U2 = vmax3(pXZ, sXY, sYZ), U3 = vmax3(pXZ, sYZ, sXZ);
    const h2 W = vmax3(U1, sYZ, sM);
    const h2 WO = W - O, WO2 = W - O2;
    p.W[i] = U(W);
    p.N1[i] = U(vmax3(X - E2, U1 - OE, WO2));
    p.N2[i] = U(hmax(U2 - OE, WO2));
    p.N3[i] = U(vmax3(Z - E2, U3 - OE, WO2));
    p.N4[i] = U(hmax(hmax(X, sXY) - E, WO));
    p.N5[i] = U(hmax(hmax(sYZ, Z) - E, WO));
    p.N6[i] = U(hmax(hmax(pXZ, sXZ) - E, WO));
  }
}
template <int M>
__device__ __forceinline__ void lap_post_f16(const PencilArgs &pa, const uint32_t (&Y)[M],
                                             const LapPre<M> &p, uint32_t (&nIx)[M],
                                             uint32_t (&oIy)[M], uint32_t (&oIz)[M],
                                             uint32_t (&oIxy)[M], uint32_t (&oIyz)[M],
                                             uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
  const h2 E = H(pa.E), O = H(pa.O), E2 = H(pa.E2), OE = H(pa.OE);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const h2 y = H(Y[i]), yOE = y - OE, yE = y - E;
    oBest[i] = U(hmax(y, H(p.W[i])));
    nIx[i] = U(hmax(yOE, H(p.N1[i])));
    oIy[i] = U(hmax(y - E2, H(p.N2[i])));
    oIz[i] = U(hmax(yOE, H(p.N3[i])));
    oIxy[i] = U(hmax(yE, H(p.N4[i])));
    oIyz[i] = U(hmax(yE, H(p.N5[i])));
    oIxz[i] = U(hmax(y - O, H(p.N6[i])));
  }
}
// The V-space cell (cell_messages_vs: every value of cell (x,y,z) shifted by
// lam (x+y+z), lam = GE = -MISMATCH) split at the row above the same way.
// With Gx = max(Y, gx), Gz = max(Y, gz), best = max(Y, W) and DO = GO - GE
// >= 0, CP = GO + MISMATCH + lam >= lam (tests/test_cell_algebra.py):
//   W  = max(gx, Gy, XY', M'),  gx = max(Z, YZ'), gz = max(X, XY'), Gy = max(X, Z, XZ')
//   Ixy' = max(Y, NXY),      NXY = max(gz, W - DO)
//   Iyz' = max(Y, NYZ),      NYZ = max(gx, W - DO)
//   Ixz' = max(Y - DO, NXZ), NXZ = max(Gy, W - DO)
//   Ix'  = max(Y - CP, N1),  N1 = max(X - lam, NXY - CP, NXZ - CP)
//   Iy'  = max(Y - lam, N2), N2 = max(NXY - CP, NYZ - CP)
//   Iz'  = max(Y - CP, N3),  N3 = max(Z - lam, NYZ - CP, NXZ - CP)
// 23 instructions per pair before the record lands, 10 after (the message
// form: 32 + 11). LapPre slots: N4 = NXY, N5 = NYZ, N6 = NXZ.
template <int M, bool SOP>
__device__ __forceinline__ void lap_pre_vs(const uint32_t (&a)[M], const uint32_t (&b)[M],
                                           const uint32_t (&c)[M], const uint32_t (&SBC)[M],
                                           const uint32_t (&K)[M], const uint32_t (&DMC)[M],
                                           const uint32_t (&DMB)[M], const PencilArgs &pa,
                                           const uint32_t (&inIx)[M], const uint32_t (&inIz)[M],
                                           const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M],
                                           const uint32_t (&inIxz)[M], const uint32_t (&inM)[M],
                                           LapPre<M> &p) {
  const h2 LAM = H(pa.v_lam), CP = H(pa.v_cP), DO = H(pa.v_dO);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const h2 eab = H(a[i] & b[i]), eac = H(a[i] & c[i]), DMCi = H(DMC[i]), DMBi = H(DMB[i]);
    const h2 sXY = hfma(eab, DMBi, H(inIxy[i]));  // src/PE_1cyc.v:159-161 (+mismatch folded)
    const h2 sXZ = hfma(eac, DMCi, H(inIxz[i]));
    const h2 sYZ = H(inIyz[i]) + H(SBC[i]);
    h2 sM;                                        // src/PE_1cyc.v:162
    if constexpr (SOP) sM = hfma(eab, DMBi, hfma(eac, DMCi, H(inM[i]))) + H(K[i]);
    else sM = hfma(eab, H(K[i]), H(inM[i]));      // ne + 3 lam = 0
    const h2 X = H(inIx[i]), Z = H(inIz[i]);
    const h2 gx = hmax(Z, sYZ), gz = hmax(X, sXY), Gy = vmax3(X, Z, sXZ);
    const h2 W = vmax3(gx, Gy, hmax(sXY, sM));
    const h2 WD = W - DO;
    const h2 NXY = hmax(gz, WD), NYZ = hmax(gx, WD), NXZ = hmax(Gy, WD);
    const h2 qXY = NXY - CP, qYZ = NYZ - CP, qXZ = NXZ - CP;
    p.W[i] = U(W);
    p.N4[i] = U(NXY);
    p.N5[i] = U(NYZ);
    p.N6[i] = U(NXZ);
    p.N1[i] = U(vmax3(X - LAM, qXY, qXZ));
    p.N2[i] = U(hmax(qXY, qYZ));
    p.N3[i] = U(vmax3(Z - LAM, qYZ, qXZ));
  }
}
template <int M>
__device__ __forceinline__ void lap_post_vs(const PencilArgs &pa, const uint32_t (&Y)[M],
                                            const LapPre<M> &p, uint32_t (&nIx)[M],
                                            uint32_t (&oIy)[M], uint32_t (&oIz)[M],
                                            uint32_t (&oIxy)[M], uint32_t (&oIyz)[M],
                                            uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
  const h2 LAM = H(pa.v_lam), CP = H(pa.v_cP), DO = H(pa.v_dO);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const h2 y = H(Y[i]), yCP = y - CP;
    oBest[i] = U(hmax(y, H(p.W[i])));
    oIxy[i] = U(hmax(y, H(p.N4[i])));
    oIyz[i] = U(hmax(y, H(p.N5[i])));
    oIxz[i] = U(hmax(y - DO, H(p.N6[i])));
    nIx[i] = U(hmax(yCP, H(p.N1[i])));
    oIy[i] = U(hmax(y - LAM, H(p.N2[i])));
    oIz[i] = U(hmax(yCP, H(p.N3[i])));
  }
}
// int16 form (two's complement halves): the same split of cell_messages
template <int M, bool SOP>
__device__ __forceinline__ void lap_pre_i16(const uint32_t (&a)[M], const uint32_t (&b)[M],
                                            const uint32_t (&c)[M], uint32_t ones,
                                            const PencilArgs &pa, const uint32_t (&inIx)[M],
                                            const uint32_t (&inIz)[M], const uint32_t (&inIxy)[M],
                                            const uint32_t (&inIyz)[M], const uint32_t (&inIxz)[M],
                                            const uint32_t (&inM)[M], LapPre<M> &p) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const uint32_t eab = pk_eq1(a[i], b[i], ones);
    const uint32_t eac = pk_eq1(a[i], c[i], ones);
    const uint32_t ebc = pk_eq1(b[i], c[i], ones);
    const uint32_t s2ab = pk_mad(eab, pa.dm, pa.mm);
    const uint32_t s2ac = pk_mad(eac, pa.dm, pa.mm);
    const uint32_t s2bc = pk_mad(ebc, pa.dm, pa.mm);
    uint32_t s3;
    if constexpr (SOP) s3 = pk_add(pk_add(s2ab, s2bc), s2ac);
    else s3 = pk_mad(eab, pk_mad(ebc, pa.s3_d1, pa.s3_d0), pa.s3_ne);
    const uint32_t sM = pk_add(inM[i], s3), X = inIx[i], Z = inIz[i];
    const uint32_t sXY = pk_add(inIxy[i], s2ab), sYZ = pk_add(inIyz[i], s2bc);
    const uint32_t sXZ = pk_add(inIxz[i], s2ac);
    const uint32_t pXZ = pk_max(X, Z);
    const uint32_t U1 = pk_max(pk_max(pXZ, sXY), sXZ), U2 = pk_max(pk_max(pXZ, sXY), sYZ);
    const uint32_t U3 = pk_max(pk_max(pXZ, sYZ), sXZ), W = pk_max(pk_max(U1, sYZ), sM);
    const uint32_t WO = pk_sub(W, pa.O), WO2 = pk_sub(W, pa.O2);
    p.W[i] = W;
    p.N1[i] = pk_max(pk_max(pk_sub(X, pa.E2), pk_sub(U1, pa.OE)), WO2);
    p.N2[i] = pk_max(pk_sub(U2, pa.OE), WO2);
    p.N3[i] = pk_max(pk_max(pk_sub(Z, pa.E2), pk_sub(U3, pa.OE)), WO2);
    p.N4[i] = pk_max(pk_sub(pk_max(X, sXY), pa.E), WO);
    p.N5[i] = pk_max(pk_sub(pk_max(sYZ, Z), pa.E), WO);
    p.N6[i] = pk_max(pk_sub(pk_max(pXZ, sXZ), pa.E), WO);
  }
}
template <int M>
__device__ __forceinline__ void lap_post_i16(const PencilArgs &pa, const uint32_t (&Y)[M],
                                             const LapPre<M> &p, uint32_t (&nIx)[M],
                                             uint32_t (&oIy)[M], uint32_t (&oIz)[M],
                                             uint32_t (&oIxy)[M], uint32_t (&oIyz)[M],
                                             uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const uint32_t y = Y[i], yOE = pk_sub(y, pa.OE), yE = pk_sub(y, pa.E);
    oBest[i] = pk_max(y, p.W[i]);
    nIx[i] = pk_max(yOE, p.N1[i]);
    oIy[i] = pk_max(pk_sub(y, pa.E2), p.N2[i]);
    oIz[i] = pk_max(yOE, p.N3[i]);
    oIxy[i] = pk_max(yE, p.N4[i]);
    oIyz[i] = pk_max(yE, p.N5[i]);
    oIxz[i] = pk_max(pk_sub(y, pa.O), p.N6[i]);
  }
}

// LIT: the literal push-form cell (literal_kernel.hip:push_literal, the RTL's
// src/PE_1cyc.v:164-218 with every candidate wrapped at SCORE_BITS), split at
// the row above the same way: every candidate but Y's is maxed before the
// record lands, Y's seven after it (13 instructions per pair). an / bn / cn:
// the successors' symbol codes (a_{x'+1}, b_{y+1}, c_{z+1}); UYZ = s2(b_{y+1},
// c_{z+1}) - GE and K1 (the [b=c] part of s3) are per-position constants.
template <int M>
struct LitPre {
  uint32_t pIx[M], pIy[M], pIz[M], pIxy[M], pIyz[M], pIxz[M], pM[M], uxy[M], vxz[M], s3[M];
};
template <int M, bool SOP>
__device__ __forceinline__ void lit_pre(const LitArgs &c, const LitArgs &cv, uint32_t ones,
                                        const uint32_t (&an)[M], uint32_t bn, const uint32_t (&cn)[M],
                                        const uint32_t (&UYZ)[M], const uint32_t (&K1)[M],
                                        const uint32_t (&X)[M], const uint32_t (&Z)[M],
                                        const uint32_t (&XY)[M], const uint32_t (&YZ)[M],
                                        const uint32_t (&XZ)[M], const uint32_t (&MM)[M], LitPre<M> &p) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    // single targets, less Y's candidates (src/PE_1cyc.v:172-194)
    const uint32_t m2O = pk_add(MM[i], c.n2O);
    const uint32_t x2E = pk_add(X[i], c.n2E), xOE = pk_add(X[i], c.nOE);
    const uint32_t z2E = pk_add(Z[i], c.n2E), zOE = pk_add(Z[i], c.nOE);
    const uint32_t xyOE = pk_add(XY[i], c.nOE), xy2O = pk_add(XY[i], c.n2O);
    const uint32_t yzOE = pk_add(YZ[i], c.nOE), yz2O = pk_add(YZ[i], c.n2O);
    const uint32_t xzOE = pk_add(XZ[i], c.nOE), xz2O = pk_add(XZ[i], c.n2O);
    const uint32_t A = pk_max(pk_max(m2O, zOE), xyOE), Bv = pk_max(xOE, yzOE);
    p.pIx[i] = pk_max(pk_max(A, x2E), pk_max(yz2O, xzOE));
    p.pIy[i] = pk_max(pk_max(A, Bv), xz2O);
    p.pIz[i] = pk_max(pk_max(Bv, m2O), pk_max(z2E, pk_max(xy2O, xzOE)));
    // the successors' pair scores less GE (u) and less GO (v), src/PE_1cyc.v:159-161
    const uint32_t eab = pk_eq1(an[i], bn, ones), eac = pk_eq1(an[i], cn[i], ones);
    const uint32_t uxy = pk_mad(eab, cv.dmS, cv.mmE), vxy = pk_add(uxy, c.nDOE);
    const uint32_t uxz = pk_mad(eac, cv.dmS, cv.mmE), vxz = pk_add(uxz, c.nDOE);
    const uint32_t uyz = UYZ[i], vyz = pk_add(uyz, c.nDOE);
    p.pIxy[i] = pk_max(pk_max(pk_max(pk_add(X[i], uxy), pk_add(XY[i], uxy)), pk_max(pk_add(MM[i], vxy), pk_add(Z[i], vxy))),
                       pk_max(pk_add(YZ[i], vxy), pk_add(XZ[i], vxy)));
    p.pIyz[i] = pk_max(pk_max(pk_max(pk_add(Z[i], uyz), pk_add(YZ[i], uyz)), pk_max(pk_add(MM[i], vyz), pk_add(X[i], vyz))),
                       pk_max(pk_add(XY[i], vyz), pk_add(XZ[i], vyz)));
    p.pIxz[i] = pk_max(pk_max(pk_max(pk_add(X[i], uxz), pk_add(Z[i], uxz)), pk_max(pk_add(XZ[i], uxz), pk_add(MM[i], vxz))),
                       pk_max(pk_add(XY[i], vxz), pk_add(YZ[i], vxz)));
    // M: every state plus the successor's triple score (src/PE_1cyc.v:162-170)
    uint32_t s3;
    if constexpr (SOP) s3 = pk_mad(eab, cv.dmS, pk_mad(eac, cv.dmS, K1[i]));
    else s3 = pk_mad(eab, K1[i], cv.neS);
    p.pM[i] = pk_max(pk_max(pk_max(pk_add(MM[i], s3), pk_add(X[i], s3)), pk_max(pk_add(Z[i], s3), pk_add(XY[i], s3))),
                     pk_max(pk_add(YZ[i], s3), pk_add(XZ[i], s3)));
    p.uxy[i] = uxy;
    p.vxz[i] = vxz;
    p.s3[i] = s3;
  }
}
template <int M>
__device__ __forceinline__ void lit_post(const LitArgs &c, const uint32_t (&Y)[M], const uint32_t (&UYZ)[M],
                                         const LitPre<M> &p, uint32_t (&nIx)[M], uint32_t (&oIy)[M],
                                         uint32_t (&oIz)[M], uint32_t (&oIxy)[M], uint32_t (&oIyz)[M],
                                         uint32_t (&oIxz)[M], uint32_t (&oM)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const uint32_t y = Y[i], yOE = pk_add(y, c.nOE);
    nIx[i] = pk_max(p.pIx[i], yOE);
    oIy[i] = pk_max(p.pIy[i], pk_add(y, c.n2E));
    oIz[i] = pk_max(p.pIz[i], yOE);
    oIxy[i] = pk_max(p.pIxy[i], pk_add(y, p.uxy[i]));
    oIyz[i] = pk_max(p.pIyz[i], pk_add(y, UYZ[i]));
    oIxz[i] = pk_max(p.pIxz[i], pk_add(y, p.vxz[i]));
    oM[i] = pk_max(p.pM[i], pk_add(y, p.s3[i]));
  }
}
// A zero cell's pushes (the faces) into a pair target and into M, per half:
// s2 of the successor's pair as fP[0] / fP[1], and s3 wrapped (P[M][*] = 0)
__device__ __forceinline__ uint32_t lit_face_pair(const LitArgs &cv, uint32_t p, uint32_t q, uint32_t ones) {
  return pk_mad(pk_eq1(p, q, ones), pk_sub(cv.fP[1], cv.fP[0]), cv.fP[0]);
}
template <bool SOP>
__device__ __forceinline__ uint32_t lit_face_m(const LitArgs &cv, uint32_t an, uint32_t bn, uint32_t cn,
                                               uint32_t ones) {
  const uint32_t eab = pk_eq1(an, bn, ones), ebc = pk_eq1(bn, cn, ones), eac = pk_eq1(an, cn, ones);
  if constexpr (SOP) return pk_mad(eab, cv.dmS, pk_mad(ebc, cv.dmS, pk_mad(eac, cv.dmS, cv.mm3S)));
  else return pk_mad(eab, pk_mad(ebc, cv.d1S, cv.d0S), cv.neS);
}

// LDS (bytes):
//   xr    [NW-1][K][M][64][16]  wave w -> w+1 records {Iy, Ixy, Iyz, best}
//   xr0   [K0][M][64][16]       tagged y records of the lap above (loader, LDS-DMA)
//   zring [ZL][NW][32]          tagged z records of the tile to the left (loader)
//   yface [M][64][16]           y = 0 face in wave 0's record format (lap 0)
//   zface [NW][32]              z = 0 face in the z record format (tile 0)
//   wd    [16] i32              [9] back-pressure waits, [12] abort, [13..14] the
//                               consumers' progress (LDS-DMA'd), [15] loader stalls
//   pw    [NW+1][64] i32        progress words (steps done): compute wave w, loader NW
//   fin   [M][64] u32           best of the final step (LIT: [7][M][64] its input
//                               states, then the 7 unshifted values)
//   sA2   [..] u32              A code pairs: entry j = x j-OFF (lo), j-OFF-1 (hi)
// Minimum waves per SIMD the register allocation must allow. A workgroup's
// NW + 1 waves may sit ceil((NW + 1) / 4) to a SIMD (the dispatcher need not
// balance them), so two NW = 8 workgroups per CU need 6 waves per SIMD, i.e.
// <= 80 VGPRs: with 96 (5 waves) the CU admitted one, and the second half of
// a 1024^3 lap grid started only as the first half finished (ring-lag census,
// profiles/r3e_lap_lag.jsonl). M = 1 keeps 6 for the plain forms (the int16
// one needs the cap to stay two per CU, tests/test_kernel_meta.py) and asks
// for 4 for the checked and literal ones, which spill 8 bytes at 6; the f16
// single cubes stay <= 80 VGPRs either way and ran alike (same box: 64^3
// 0.0741 ms at 4 vs 0.0748 at 6, 256^3 0.351 vs 0.356; without the per-lap
// index launder (TSA_LAP_LAUNDER=0) 256^3 0.366, profiles/r4j_single_ab.jsonl).
// M >= 4 runs one per CU.
#ifndef TSA_LAP_WPE2
#define TSA_LAP_WPE2 4
#endif
#ifndef TSA_LAP_WPE2C  // the checked M = 2 form (5: 1024^3 3.38 vs 3.24 ms, profiles/r4q_checked_ab.jsonl)
#define TSA_LAP_WPE2C 4
#endif
#ifndef TSA_LAP_LAUNDER
#define TSA_LAP_LAUNDER 1
#endif
#ifndef TSA_LAP_WPE1
#define TSA_LAP_WPE1 6
#endif
// The checked kernel's monitor: per-wave slots written with plain stores and
// reduced per triple by lap_certify (1), or two same-address atomics per wave
// (0, rounds 1-4). Thousands of waves of one cube contend for the two words,
// and a looped workgroup waits for its atomics (vmcnt(0)) before its next lap.
#ifndef TSA_CHK_SLOTS
#define TSA_CHK_SLOTS 1
#endif
// Lean step: the producer's progress word read every step (no poll flag kept
// in a VGPR across the pre-cell, no conditional read), and the next A codes
// at a constant offset from a base set once per step pair
#ifndef TSA_LAP_LEAN
#define TSA_LAP_LEAN 1
#endif
// wave 0 reads only the payload words of its tagged y record (ds_read2_b32):
// a 16-byte read hands the compiler the two dead tag registers, which it
// reuses before the read has landed -- a write-after-write wait that puts
// the record read's latency in front of the pre-cell
#ifndef TSA_LAP_Y2  // (measured: 64^3 / 256^3 / 512^3 0.5-1 % faster, profiles/r5a_lap_y2_ab.jsonl)
#define TSA_LAP_Y2 1
#endif
// Four-step groups: a step's ring slots, z / y record addresses and next A
// codes sit at constant offsets (instruction immediates) from bases set once
// per group of four steps -- every ring length is a multiple of 4 and ZT of
// LAP_ZL -- instead of being computed every step. The message forms' constant
// y = 0 / z = 0 faces are prefilled into every slot of xr0 / zring (which the
// loader then leaves alone), so the offsets never depend on yin / zin.
#ifndef TSA_LAP_U4
#define TSA_LAP_U4 1
#endif
// In a four-step group, the back-pressure checks batched: the consumers' ring
// room once per group (for its last step; the rings hold >= 32 slots), the
// successor wave's slot every other step for K = 4 (covering the next step:
// it needs the successor past step t - 2 at the end of step t, which it
// normally is, one step behind)
#ifndef TSA_LAP_GCHK
#define TSA_LAP_GCHK 1
#endif
// In a four-step group, every LDS base a step reads or writes (the input and
// output record rings, the group's y / z ring slots, the two progress words)
// held in a VGPR laundered once per lap / group, so each access is one ds
// instruction with a constant offset; left alone the compiler keeps the
// uniform part in SGPRs -- one per ring slot, spilled to VGPR lanes -- and
// rebuilds every address with v_readlane / v_mov / v_add each step. The ring
// records go out through the SGPR-base form of global_store (no 64-bit VGPR
// address per store).
#ifndef TSA_LAP_VBASE
#define TSA_LAP_VBASE 1
#endif
// The loader fetches each ring record (two {payload, tag} granules) with one
// 16-byte load instead of two 8-byte ones: 2M + 2 load instructions per step
// become M + 1 (plus the progress words). 0: two 8-byte atomic loads; 1: a
// volatile 16-byte load (measured 1.8x slower: the memory legalizer follows
// each volatile load with vmcnt(0), serialising the fetch window,
// profiles/r5f_lap_loader_ab.jsonl); 2: a raw buffer load with sc1 (counted by
// the compiler like the atomics); -1 (default): 2 for the M = 1 forms, 0 for
// the rest (with the progress words every 4 steps: factored 64^3 / 256^3 /
// 512^3 5-6 % faster, profiles/r5i_lap_loader_ab.jsonl; literal 512^3 / 1024^3
// 5 / 4 % faster, r5j_lap_loader_lit_ab.jsonl; the M = 2 checked 1024^3
// neutral)
#ifndef TSA_LAP_L16
#define TSA_LAP_L16 -1
#endif
// The consumers' progress words (the producers' back-pressure input, relayed
// through LDS) fetched once per loader period instead of every step: fewer
// loads in the loader's window (the consumers publish every LAP_PUB = 4 steps
// anyway; a staler relay only waits more, never less). The loader loop runs in
// periods of LU steps with a static phase, LU = PROGP when PROGP is a multiple
// of LPD above it, else LPD -- so the EFFECTIVE refresh period is LU (with
// PROGP = 2 and LPD = 3, as the M = 4 forms have, every 3 steps, not 2). -1
// (default): PROGP 4 for the M = 1 forms (LPD 2: every 4 steps), 2 for the rest
// (LPD 2: every 2 steps) (profiles/r5h_lap_prog_ab.jsonl,
// r5i_lap_loader_ab.jsonl, r5j_lap_loader_lit_ab.jsonl).
#ifndef TSA_LAP_PROGP
#define TSA_LAP_PROGP -1
#endif
// With the buffer loads (TSA_LAP_L16 = 2): the fetches a lap-0 / tile-0 loader
// does not need (its y / z inputs are faces) out of range, so no memory access
// (measured neutral: 64^3 - 512^3 within 0.5 %, profiles/r5j_lap_noface_ab.jsonl)
#ifndef TSA_LAP_NOFACE_FETCH
#define TSA_LAP_NOFACE_FETCH 1
#endif
__host__ __device__ constexpr int lap_waves_per_eu(int M, bool lit = false, bool chk = false) {
  return lit ? (M == 1 ? 4 : 3) : M == 1 ? (chk ? 4 : TSA_LAP_WPE1) : M == 2 ? (chk ? TSA_LAP_WPE2C : TSA_LAP_WPE2) : 2;
}
// f(integral_constant<J>) for J = B .. E-1, unrolled at compile time
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
// every step of the lap kernel inlined (outlined, the captures go to scratch)
#define LAP_INLINE(call) \
  do {                    \
    [[clang::always_inline]] call; \
  } while (0)

// CHK (int16 form only): the checked kernel -- every real cell's best is
// folded into a per-lane max / min; each wave's extremes go to its own monitor
// slots (TSA_CHK_SLOTS), and lap_certify() reduces a triple's and decides whether
// any candidate of the literal RTL recurrence could have wrapped.
// A launch runs laps [L0, L1) of the cube (a single launch: [0, G)). SYS: one
// part of a cube split over devices (lap_launch_split) -- every hand-off load
// and store at system scope, the y ring of lap L1-1 written into the next
// part's workspace (yf_out, its consumer's memory) and the progress words of
// lap L0 into the previous part's (prog_in, its producer's memory), so every
// poll reads local memory and only posted stores cross the link.
// LIT: the literal RTL arithmetic (tools/litlap_emu.py replays it): the push-
// form cell of the literal helix on this schedule -- a position computes
// x' = u (x' = 0 the x = 0 face: its 7 inputs forced to 0, one more step), it
// pushes with its successors' symbols, the loader writes the y = 0 / z = 0
// faces (zero cells pushing with the receivers' symbols, so they vary with the
// step) into the rings wave 0 and position 0 read, values are shifted left by
// 16 - SCORE_BITS so int16 adds wrap at the RTL word, and the final cell's 7
// input states go to mon (aux) as its final 7-tuple.
// The kernel's arguments, bundled on the host and passed as separate
// __restrict__ parameters (LAP_KARGS). Measured: one by-value struct read
// through the kernarg segment pointer ran single cubes 15 % slower (64^3 0.087
// vs 0.075 ms, 256^3 0.40 vs 0.355 ms, same box, profiles/r4i_single_ab.jsonl)
// -- likely the no-alias guarantee the parameters carry and the fields do not.
struct LapKArgs {
  const uint8_t *seqs;
  const int64_t *offs;
  int32_t G, GZ, NC, CH, YR, ZR;
  uint8_t *yf_base, *zf_base;
  LapRounds rd;
  int32_t *prog;
  uint32_t *err;
  int32_t *scores, *mon;
  PencilArgs pa;
  uint32_t epoch, spin_limit;
  int32_t L0, L1;
  uint8_t *yf_out;
  int32_t *prog_in;
  unsigned long long *trace;
  LitArgs lit;
};
#define LAP_KARGS(k)                                                                                   \
  k.seqs, k.offs, k.G, k.GZ, k.NC, k.CH, k.YR, k.ZR, k.yf_base, k.zf_base, k.rd, k.prog, k.err, k.scores, \
      k.mon, k.pa, k.epoch, k.spin_limit, k.L0, k.L1, k.yf_out, k.prog_in, k.trace, k.lit
// VS: the V-space f16 cell (lap_pre_vs), every value shifted by lam (x+y+z):
// the faces become lam q (the x = 0 face injected at x = 1, the y = 0 / z = 0
// faces written by the loader like the literal form's), the score shifted
// back at the end.
// The end search's per-lane state: the running key of half h of register i,
// the first x - 1 at which that half is a candidate (0, or la - 1 under
// pa.end_face off the end faces) and the lane's step offset 2w + M lane.
// Empty unless END (as the helix's EndKeys, pencil_kernel.hip): unused plain
// locals captured by the step lambda still cost the other forms registers.
template <int M, bool END>
struct LapEndKeys {
  uint32_t v[2][M];
  int32_t xlo[2][M];
  int32_t kb;
};
template <int M>
struct LapEndKeys<M, false> {};
constexpr int32_t LAP_END_XMAX = 0xFFFE;  // x - 1 the key's 16 bits hold (a real cell's key is never 0)

// The body of both __global__ forms below is lap_kernel_body.h, included inside
// each: the same text for both, so the score kernels' code does not depend on
// the end search's (an inlined function template shared by two wrappers moved
// eight of their register counts).
template <int M, int NW, bool F16, bool SOP, bool CHK, bool SYS = false, bool LIT = false, bool VS = false>
__global__ __launch_bounds__(64 * (NW + 1), lap_waves_per_eu(M, LIT, CHK)) void lap_kernel(
    const uint8_t *__restrict__ seqs_, const int64_t *__restrict__ offs_, int32_t G_, int32_t GZ_,
    int32_t NC_, int32_t CH_, int32_t YR_, int32_t ZR_, uint8_t *__restrict__ yf_base_,
    uint8_t *__restrict__ zf_base_, LapRounds rd_, int32_t *__restrict__ prog_, uint32_t *__restrict__ err_,
    int32_t *__restrict__ scores_, int32_t *__restrict__ mon_, PencilArgs pa_, uint32_t epoch_,
    uint32_t spin_limit_, int32_t L0_, int32_t L1_, uint8_t *__restrict__ yf_out_,
    int32_t *__restrict__ prog_in_, unsigned long long *__restrict__ trace_, LitArgs lit_) {
  constexpr bool END = false;
  constexpr unsigned long long *ekey_ = nullptr;
#include "lap_kernel_body.h"
}

// END (the checked int16 form only; lap_ends_kernel, tsa_score_batch_ends_lap):
// the end-free score. Row y and position z of a register half stay fixed for
// the whole lap and only x = t - (2w + h) - (M lane + i) + 1 moves, ascending,
// so every half keeps one 32-bit key {best ^ 0x8000 : 0xFFFF - (x - 1)} of its
// candidate cells, folded with an unsigned max: the largest score, then the
// smallest x, whatever the order of folding. A candidate is a cell with
// 0 <= x - 1 < la (the monitor's mask lets the cells not yet started and the
// drain cells past x = la through; the end search must not) of a real row and
// a real position -- those two are constants of the half, applied once after
// the step loop. pa.end_face: only the row y = lb and the position z = lc keep
// the whole x range, every other half is a candidate at x = la alone. After
// the loop a lane widens its keys by ~(y - 1) and ~(z - 1), the wave reduces
// them, and lane 0 stores the wave's key into its slot of ekey (beside its
// monitor slots, a plain store); lap_ends_reduce takes a triple's largest.
// ekey_: the key slots, one per compute wave of every logical workgroup. A
// __global__ name of its own, so its registers bound its own plans
// (lap_ends_simd_blocks_per_cu) and not the score plans of lap_kernel.
template <int M, int NW, bool SOP>
__global__ __launch_bounds__(64 * (NW + 1), lap_waves_per_eu(M, false, true)) void lap_ends_kernel(
    const uint8_t *__restrict__ seqs_, const int64_t *__restrict__ offs_, int32_t G_, int32_t GZ_,
    int32_t NC_, int32_t CH_, int32_t YR_, int32_t ZR_, uint8_t *__restrict__ yf_base_,
    uint8_t *__restrict__ zf_base_, LapRounds rd_, int32_t *__restrict__ prog_, uint32_t *__restrict__ err_,
    int32_t *__restrict__ scores_, int32_t *__restrict__ mon_, PencilArgs pa_, uint32_t epoch_,
    uint32_t spin_limit_, int32_t L0_, int32_t L1_, uint8_t *__restrict__ yf_out_,
    int32_t *__restrict__ prog_in_, unsigned long long *__restrict__ trace_, LitArgs lit_,
    unsigned long long *__restrict__ ekey_) {
  constexpr bool F16 = false, CHK = true, SYS = false, LIT = false, VS = false, END = true;
#include "lap_kernel_body.h"
}

// Certification of the checked kernel's triples: a score stands when every
// best it saw lies in [best_min, best_max]. TSA_CHK_SLOTS: one workgroup per
// triple reduces its per_tri wave slots ([max] at mon, [min] at mon + nslot;
// slots of waves that did not run keep the launch's neutral fill); otherwise
// one thread per triple reads its two atomic words.
__global__ __launch_bounds__(256) void lap_certify(const int32_t *__restrict__ mon, int32_t n, int64_t nslot,
                                                   int32_t per_tri, CheckLimits lim, int32_t *__restrict__ scores) {
  if constexpr (TSA_CHK_SLOTS) {
    __shared__ int32_t red[2][4];
    const int32_t i = blockIdx.x;
    const int64_t base = (int64_t)i * per_tri;
    int32_t mx = INT32_MIN, mn = INT32_MAX;
    for (int32_t j = threadIdx.x; j < per_tri; j += 256) {
      mx = max(mx, mon[base + j]);
      mn = min(mn, mon[nslot + base + j]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mx = max(mx, __shfl_xor(mx, d));
      mn = min(mn, __shfl_xor(mn, d));
    }
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = mx;
      red[1][threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      mx = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
      mn = min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3]));
      if ((mx > lim.best_max || mn < lim.best_min) && scores[i] != TSA_SCORE_INVALID)
        scores[i] = TSA_SCORE_UNCERTIFIED;
    }
  } else {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (mon[i] > lim.best_max || mon[n + i] < lim.best_min) {
      if (scores[i] != TSA_SCORE_INVALID) scores[i] = TSA_SCORE_UNCERTIFIED;
    }
  }
}

// The end search's reduction (lap_ends_kernel's launches), one workgroup per
// triple: the largest of its per_tri key slots gives the score and the end
// cell (the key orders cells by score, then the smaller x, y, z); its monitor
// slots are reduced as lap_certify does. A launch whose hand-off timed out
// (*err == epoch) reads TSA_SCORE_INVALID, a triple outside lim
// TSA_SCORE_UNCERTIFIED, both with ends 0, 0, 0. Slots of waves that did not
// run keep the launch's neutral fill (key 0).
__global__ __launch_bounds__(256) void lap_ends_reduce(const int32_t *__restrict__ mon,
                                                       const unsigned long long *__restrict__ ekey, int64_t nslot,
                                                       int32_t per_tri, CheckLimits lim,
                                                       const uint32_t *__restrict__ err, uint32_t epoch,
                                                       int32_t *__restrict__ scores, int32_t *__restrict__ ends) {
  __shared__ int32_t red[2][4];
  __shared__ unsigned long long redk[4];
  const int32_t i = blockIdx.x;
  const int64_t base = (int64_t)i * per_tri;
  int32_t mx = INT32_MIN, mn = INT32_MAX;
  unsigned long long bk = 0ull;
  for (int32_t j = threadIdx.x; j < per_tri; j += 256) {
    mx = max(mx, mon[base + j]);
    mn = min(mn, mon[nslot + base + j]);
    bk = max(bk, ekey[base + j]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mx = max(mx, __shfl_xor(mx, d));
    mn = min(mn, __shfl_xor(mn, d));
    bk = max(bk, (unsigned long long)__shfl_xor(bk, d));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mx;
    red[1][threadIdx.x >> 6] = mn;
    redk[threadIdx.x >> 6] = bk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
    mn = min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3]));
    bk = max(max(redk[0], redk[1]), max(redk[2], redk[3]));
    int32_t s, e[3] = {0, 0, 0};
    if (*err == epoch || bk == 0ull) {
      s = TSA_SCORE_INVALID;
    } else if (mx > lim.best_max || mn < lim.best_min) {
      s = TSA_SCORE_UNCERTIFIED;
    } else {
      s = (int32_t)(int16_t)(uint16_t)((bk >> 48) ^ 0x8000u);
      for (int k = 0; k < 3; ++k) e[k] = 0xFFFF - (int32_t)((bk >> (32 - 16 * k)) & 0xFFFFu) + 1;
    }
    scores[i] = s;
    for (int k = 0; k < 3; ++k) ends[3 * (int64_t)i + k] = e[k];
  }
}

// ---------------------------------------------------------------------------
// Host planning.

// Per-device facts the residency check needs, read once per device.
struct DevInfo {
  int cus = 256;
  bool known = false;
};
static DevInfo dev_info() {
  static DevInfo cache[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return DevInfo{};
  if (!cache[d].known) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && cus > 0)
      cache[d].cus = cus;
    cache[d].known = true;
  }
  return cache[d];
}

// The register bound on lap workgroups per CU: waves per SIMD the SGPR and
// VGPR files admit (build-time kernel table, kernel_meta.h), a workgroup of
// NW + 1 waves taking up to ceil((NW + 1) / 4) of them on one SIMD. The
// occupancy API counts waves per CU instead and reads one workgroup high at
// the SGPR edge (MI355X_MICROARCH.md:463) and, measured, at 96 VGPRs with
// 9-wave workgroups (it said 2, the CU ran 1).
// The bound is taken over every instantiation of the shape and form -- the
// checked (CHK) and split (SYS) ones too, whose register counts can differ
// from the plain kernel's -- so the grid plan holds whichever of them runs.
int lap_simd_blocks_per_cu(int M, int NW, bool f16, bool sop, bool lit) {
  // memo (value + 1; 0 = not yet computed): the table scans run per plan
  static std::atomic<int> memo[4][2][2][2][2];
  const int mi = M == 1 ? 0 : M == 2 ? 1 : M == 4 ? 2 : 3;
  std::atomic<int> &slot = memo[mi][NW == 8][f16][sop][lit];
  if (const int v = slot.load(std::memory_order_relaxed)) return v - 1;
  int sgpr = -1, vgpr = -1;
  for (int chk = 0; chk < 2; ++chk)
    for (int sys = 0; sys < 2; ++sys) {
      char prefix[80];  // lap_kernel<M, NW, F16, SOP, CHK, SYS, LIT>
      snprintf(prefix, sizeof prefix, "_ZN3tsa10lap_kernelILi%dELi%dELb%dELb%dELb%dELb%dELb%dE", M, NW,
               f16 ? 1 : 0, sop ? 1 : 0, chk, sys, lit ? 1 : 0);
      sgpr = std::max(sgpr, kernel_sgpr_max(prefix));
      vgpr = std::max(vgpr, kernel_vgpr_max(prefix));
    }
  const int waves = std::min(sgpr_waves_per_simd(sgpr < 0 ? 112 : sgpr), vgpr_waves_per_simd(vgpr < 0 ? 256 : vgpr));
  const int r = waves / ((NW + 1 + 3) / 4);
  slot.store(r + 1, std::memory_order_relaxed);
  return r;
}
// The same bound for the end search's kernels (lap_ends_kernel<M, NW, SOP>,
// M <= 2), from their own rows of the table: their plans size the resident
// round by it, and the score plans above do not see them.
int lap_ends_simd_blocks_per_cu(int M, int NW, bool sop) {
  char prefix[80];
  snprintf(prefix, sizeof prefix, "_ZN3tsa15lap_ends_kernelILi%dELi%dELb%dEE", M, NW, sop ? 1 : 0);
  const int sgpr = kernel_sgpr_max(prefix), vgpr = kernel_vgpr_max(prefix);
  if (sgpr < 0 || vgpr < 0) return 0;  // not instantiated
  return std::min(sgpr_waves_per_simd(sgpr), vgpr_waves_per_simd(vgpr)) / ((NW + 1 + 3) / 4);
}
// Workgroups of one shape a CU holds, from the HIP occupancy API on the real
// kernels (VGPRs, LDS) capped by the SGPR bound (the API reads one block high
// at 81-112 SGPRs); without a device, the LDS / wave-slot model. The API is
// asked about every instantiation the plan can launch -- the plain kernel, the
// checked (CHK) one of the int16 form and the V-space (VS) one of the f16
// form -- and the least count stands, so the looped grid's residency holds
// whichever of them runs. Memoized per (device, LDS bytes): a single-cube call
// plans a dozen geometries, and each occupancy query is host latency on that
// call.
template <int M, int NW, bool F16, bool SOP, bool LIT = false>
static int lap_blocks_per_cu_t(size_t lds) {
  struct Entry {
    int dev;
    size_t lds;
    int nb;
  };
  static std::mutex mu;
  static std::vector<Entry> memo;
  int nb = 0;
  int dev = -1;
  const int sg = lap_simd_blocks_per_cu(M, NW, F16, SOP, LIT);
  if (hipGetDevice(&dev) == hipSuccess) {
    {
      std::lock_guard<std::mutex> g(mu);
      for (const Entry &e : memo)
        if (e.dev == dev && e.lds == lds) return e.nb;
    }
    auto query = [&](auto kfn) -> int {
      int k = 0;
      return hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, kfn, 64 * (NW + 1), lds) == hipSuccess ? k : -1;
    };
    nb = query(lap_kernel<M, NW, F16, SOP, false, false, LIT>);
    if (nb >= 0) {
      if constexpr (!F16 && !LIT) nb = std::min(nb, std::max(0, query(lap_kernel<M, NW, false, SOP, true>)));
      if constexpr (F16 && !LIT)
        nb = std::min(nb, std::max(0, query(lap_kernel<M, NW, true, SOP, false, false, false, true>)));
      nb = std::min(nb, sg);
      std::lock_guard<std::mutex> g(mu);
      if (memo.size() < 4096) memo.push_back(Entry{dev, lds, nb});
      return nb;
    }
  }
  return (int)std::min<size_t>(std::min<size_t>(LDS_MAX / std::max<size_t>(lds, 1), 32 / (NW + 1)), sg);
}
template <int M, int NW, bool SOP>
static int lap_blocks_per_cu_lit(size_t lds) {
  return lap_blocks_per_cu_t<M, NW, false, SOP, true>(lds);
}
// The end search's kernel of that shape: the occupancy API on lap_ends_kernel
// capped by its own register bound (memoized as above).
template <int M, int NW, bool SOP>
static int lap_ends_blocks_per_cu_t(size_t lds) {
  struct Entry {
    int dev;
    size_t lds;
    int nb;
  };
  static std::mutex mu;
  static std::vector<Entry> memo;
  int dev = -1;
  const int sg = lap_ends_simd_blocks_per_cu(M, NW, SOP);
  if (hipGetDevice(&dev) == hipSuccess) {
    {
      std::lock_guard<std::mutex> g(mu);
      for (const Entry &e : memo)
        if (e.dev == dev && e.lds == lds) return e.nb;
    }
    int k = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, lap_ends_kernel<M, NW, SOP>, 64 * (NW + 1), lds) ==
        hipSuccess) {
      const int nb = std::min(k, sg);
      std::lock_guard<std::mutex> g(mu);
      if (memo.size() < 4096) memo.push_back(Entry{dev, lds, nb});
      return nb;
    }
  }
  return (int)std::min<size_t>(std::min<size_t>(LDS_MAX / std::max<size_t>(lds, 1), 32 / (NW + 1)), sg);
}
#define TSA_LAP_SHAPES(FN, M_, NW_, F16_, SOP_, ...)                                         \
  ((M_) == 1 ? ((NW_) == 4 ? TSA_ARITH(FN, 1, 4, F16_, SOP_, __VA_ARGS__)                      \
                           : TSA_ARITH(FN, 1, 8, F16_, SOP_, __VA_ARGS__))                     \
   : (M_) == 2 ? ((NW_) == 4 ? TSA_ARITH(FN, 2, 4, F16_, SOP_, __VA_ARGS__)                    \
                             : TSA_ARITH(FN, 2, 8, F16_, SOP_, __VA_ARGS__))                   \
               : ((NW_) == 4 ? TSA_ARITH(FN, 4, 4, F16_, SOP_, __VA_ARGS__)                    \
                             : TSA_ARITH(FN, 4, 8, F16_, SOP_, __VA_ARGS__)))
// The literal form's shapes: M = 1, 2 and NW = 4, 8, by s3 mode
#define TSA_LIT_SOP(FN, MM, NN, SOP_, ...) ((SOP_) ? FN<MM, NN, true>(__VA_ARGS__) : FN<MM, NN, false>(__VA_ARGS__))
#define TSA_LIT_SHAPES(FN, M_, NW_, SOP_, ...)                                                         \
  ((M_) == 1 ? ((NW_) == 4 ? TSA_LIT_SOP(FN, 1, 4, SOP_, __VA_ARGS__) : TSA_LIT_SOP(FN, 1, 8, SOP_, __VA_ARGS__)) \
             : ((NW_) == 4 ? TSA_LIT_SOP(FN, 2, 4, SOP_, __VA_ARGS__) : TSA_LIT_SOP(FN, 2, 8, SOP_, __VA_ARGS__)))

// Step time (us) along the chain, fitted on MI355X to single cubes
// (geometry sweeps profiles/r4m_lapgeo.jsonl, r4u_lap_nw.jsonl via
// scripts/gpu_lapgeo.sh; tools/lap_trace.py; DESIGN.md 4.4: 64^3..1024^3
// within ~10 %) and to batches of 4..128 cubes (profiles/r3o_chunk.jsonl:
// M = 4, 16 x 256^3 .. 4 x 1024^3), growing with the workgroups per CU -- the
// chain steps include the hand-off stalls.
// LIT: the literal cell's step, ~1.6x the message form's (single cubes and
// batches, profiles/r3l_literal_lap_vs_plane.jsonl, r3o_chunk.jsonl).
// M = 1 with two workgroups per CU (the latency-bound waves share SIMDs):
// ~0.97 us per chained step (16 x 256^3 and 1024^3 in rounds,
// profiles/r4c_lapab.jsonl), twice the one-per-CU step.
static double lap_step_us(int M, int NW, int64_t wg_per_cu, bool lit = false, bool one_round = false) {
  const double base = M == 1 ? (NW == 4 ? 0.40 : 0.49) : M == 2 ? 0.62 : 1.45;
  // per extra workgroup on the CU: two 9-wave M = 1 workgroups (4.5 waves per
  // SIMD) ~double the step; two 5-wave ones in one resident round barely slow
  // it (profiles/r4u_lap_nw.jsonl: 512^3 NW = 4 0.815 ms vs NW = 8 0.816,
  // 384^3 0.568 vs 0.599, literal 512^3 1.046 vs 1.132)
  const double share = M == 1 ? (NW == 4 && one_round ? 0.1 : 1.0) : 0.22;
  return (lit ? 1.6 : 1.0) * base * (1.0 + share * (double)(std::max<int64_t>(wg_per_cu, 1) - 1));
}

LapGeom lap_geom(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, int M, int NW,
                 bool full_rings, bool f16, bool sop, bool lit, bool ends) {
#if defined(TSA_DIAG)  // A/B knob: full-length rings (no back-pressure) on every lap launch
  if (const char *e = getenv("TSA_LAP_FULL_RINGS")) full_rings = full_rings || atoi(e) != 0;
#endif
  LapGeom g{};
  g.M = M;
  g.NW = NW;
  g.chunk = 0;
  g.max_la = max_la;
  g.max_lb = max_lb;
  g.max_lc = max_lc;
  const int RW = 2 * NW, ZT = 64 * M, LPD = lap_pd(M);
  g.G = (max_lb + RW - 1) / RW;
  g.GZ = (max_lc + ZT - 1) / ZT;
  g.NC = n * g.GZ;             // columns: (triple, z-tile)
  g.CH = (g.NC + 7) / 8;       // columns per XCD
  const int YOFF = 2 * (NW - 1) + 1;  // lap lag of a record (kernel: YOFF)
  const int32_t T = max_la + YOFF + ZT;  // >= every workgroup's step count
  auto pow2 = [](int64_t v) { int64_t p = 1; while (p < v) p <<= 1; return (int32_t)p; };
  g.lds = lap_lds_bytes(M, NW, max_la, lit);
  const int64_t wgs = (int64_t)n * g.G * g.GZ;
  if (lit && (f16 || M > 2)) return g;  // the literal form's instantiations (.ok = false)
  if (ends && (f16 || lit || M > 2)) return g;  // the end search's: int16, M <= 2
  int per_cu = (g.lds > LDS_MAX) ? 0
               : lit             ? TSA_LIT_SHAPES(lap_blocks_per_cu_lit, M, NW, sop, g.lds)
                                 : TSA_LAP_SHAPES(lap_blocks_per_cu_t, M, NW, f16, sop, g.lds);
  // the end search launches lap_ends_kernel: its own residency (never above
  // the checked score kernel's, whose workspace the geometry shares)
  if (ends && per_cu > 0) per_cu = std::min(per_cu, TSA_LIT_SHAPES(lap_ends_blocks_per_cu_t, M, NW, sop, g.lds));
  const int cus = dev_info().cus;
  // Slim rings: the lag between co-resident neighbours stays small (ring-lag
  // census, TSA_DIAG, profiles/r3e_lap_lag.jsonl): y <= 55 steps, z <= 207
  // beyond the natural ZT + ZA with one workgroup per CU; ~100 / ~200 with two
  // sharing a CU. So 32 (one per CU) or 96 slots beyond the natural lag,
  // rounded up to a power of 2. The big lags of round 2 (its workgroups start
  // as round-1 ones finish: 671 steps at 1024^3) go to the boundary rings.
  // A/B knob TSA_LAP_RING_SLACK (TSA_DIAG builds).
  int slack = (per_cu >= 2 && wgs > cus) ? 96 : 32;
#if defined(TSA_DIAG)
  if (const char *e = getenv("TSA_LAP_RING_SLACK")) slack = std::max(16, atoi(e));
#endif
  g.YR = full_rings ? pow2(T) : pow2(YOFF + LPD + slack);
  g.ZR = full_rings ? pow2(T) : pow2(ZT + LPD + slack);
  g.YRB = g.ZRB = pow2(T);
  g.blocks = (int64_t)g.G * g.CH * 8;
  // progress words, the error word (+63 spare), the checked kernel's monitor (2 n)
  // progress words, the error word (+63 spare), the checked kernel's monitor
  // (TSA_CHK_SLOTS: two words per compute wave; else two per triple)
  const size_t mon_words = TSA_CHK_SLOTS ? 2 * (size_t)wgs * NW : 2 * (size_t)n;
  g.prog_bytes = (((size_t)wgs * LAP_PROG_STRIDE + 64 + mon_words) * sizeof(int32_t) + 255) &
                 ~(size_t)255;
  g.yf_bytes = (size_t)wgs * g.YR * M * 1024;
  g.zf_bytes = (size_t)wgs * g.ZR * NW * LAP_ZREC_WAVE;
  if (g.lds > LDS_MAX || g.blocks > 0x7FFFFFFF) return g;
  // residency per XCD: block b runs on XCD b % 8 (column c's laps on XCD
  // c % 8), in block order, SX at a time (measured: tools/lap_trace.py xcc and
  // start stamps)
  const int64_t wg_per_xcd = (int64_t)g.G * g.CH;
  const int64_t slots_xcd = (int64_t)std::max(1, cus / 8) * per_cu;
  g.per_cu = per_cu;
  g.waves = per_cu > 0 ? (wg_per_xcd + slots_xcd - 1) / slots_xcd : 0;
  // dispatch rounds: boundary rings for producers whose consumer is in a later
  // round (kernel: y_bidx / z_bidx); one round, or full rings: none
  g.SX = (full_rings || g.waves <= 1 || per_cu <= 0) ? (1 << 30) : (int32_t)slots_xcd;
  g.grid = g.SX < (1 << 30) ? 8 * (int64_t)g.SX : g.blocks;  // one resident round, looped
  g.KBY = g.KBZ = 0;
  if (g.SX < (1 << 30)) {
    if (g.CH >= g.SX) {
      g.KBY = g.G;
    } else {
      for (int32_t c = 0; c < g.CH; ++c)
        g.KBY = std::max(g.KBY, ((g.G - 1) * g.CH + c) / g.SX - c / g.SX);
    }
    g.KBZ = (int32_t)g.waves;  // index: the producer's round (< rounds)
  }
  g.yb_bytes = (size_t)g.NC * g.KBY * g.YRB * M * 1024;
  g.zb_bytes = (size_t)g.KBZ * g.ZRB * NW * LAP_ZREC_WAVE;
  // one workgroup is the helix's job; a TSA_DIAG build allows it with
  // TSA_LAP_SINGLE=1 (the step time with no hand-off)
#if defined(TSA_DIAG)
  const bool single = getenv("TSA_LAP_SINGLE") && atoi(getenv("TSA_LAP_SINGLE")) != 0;
#else
  const bool single = false;
#endif
  g.ok = per_cu > 0 && (g.G >= 2 || g.GZ >= 2 || single);
  // estimated latency (us): the chain to the final workgroup -- each lap adds
  // YOFF + LPD + ~3 steps, each tile ZT + LPD + ~2 -- plus its own steps;
  // several workgroups on one CU share its SIMDs.
  const int64_t xcd_cus = std::max(1, cus / 8);
  const int64_t wg_cu = std::max<int64_t>(1, std::min<int64_t>(per_cu, (wg_per_xcd + xcd_cus - 1) / xcd_cus));
  const double steps = (double)(g.G - 1) * (YOFF + LPD + 3) + (double)(g.GZ - 1) * (ZT + LPD + 2) +
                       (double)(max_la + YOFF + ZT);
  const double step = lap_step_us(M, NW, wg_cu, lit, g.waves <= 1);
  const double chain = steps * step;
  // a slot's lap of round r + 1 starts when its lap of round r ends: one lap's
  // steps after its start, against (laps per round - 1) hand-offs of the chain
  // -- a round boundary delays the chain by the difference (round 2 of 1024^3,
  // M = 2, one workgroup per CU: 3.04 ms measured against a 2.25 ms chain)
  double delay = 0.0;
  if (g.waves > 1) {
    const double lpr = std::max(1.0, (double)g.SX / (double)g.CH);  // laps of a column per round
    const double lap_steps = (double)(max_la + YOFF + ZT) + (double)(g.GZ - 1) * (ZT + LPD + 2) / lpr;
    delay = std::max(0.0, lap_steps - (lpr - 1.0) * (YOFF + LPD + 3)) * step * 1.5;
  }
  g.est_us = chain + (double)(std::max<int64_t>(g.waves, 1) - 1) * delay;
  // refit on the round-4 runs (profiles/r4m_lapgeo.jsonl, r4j_lapab.jsonl,
  // r4t_literal_geo.jsonl): measured / estimated over several rounds is
  // 0.69-0.90 for M = 1 (1024^3 0.86, 768^3 0.90, 8 x 512^3 0.69, 16 x 256^3
  // 0.74) and 0.72-0.76 for the literal M = 1 (1024^3, 768^3), against
  // 0.84-1.15 for M = 2; the factors put 768^3 (1.90 vs 2.12 ms) and literal
  // 1024^3 (4.10 vs 4.37) on M = 1 and leave 1024^3 (2.98 vs 3.08), 8 x 512^3
  // and 16 x 256^3 on M = 2
  if (M == 1 && g.waves > 1) g.est_us *= lit ? 0.7 : 0.8;
  return g;
}

LapGeom lap_geom_chunked(int32_t n, int32_t max_la, int32_t max_lb, int32_t max_lc, int M, int NW, bool f16,
                         bool sop, bool lit, bool ends) {
  LapGeom best{};
  best.ok = false;
  int32_t forced = 0;
  long v = 0;
  if (override_int("lap_chunk", &v)) forced = (int32_t)std::max(0L, std::min(v, 1L << 30));  // plan override (tests)
  // chunk sizes n, ceil(n/2), ceil(n/4), .. 1: a later launch starts once
  // the earlier one drains (~5 us between launches on one stream)
  for (int32_t k = n;; k = (k + 1) / 2) {
    const int32_t kk = forced > 0 ? std::min(forced, n) : k;
    LapGeom g = lap_geom(kk, max_la, max_lb, max_lc, M, NW, false, f16, sop, lit, ends);
    // rounds run as each workgroup's loop over its slots (lap_kernel), in lap
    // order whatever the workgroups per CU
    if (g.ok && g.waves <= LAP_MAX_WAVES) {
      const int64_t launches = (n + kk - 1) / kk;
      g.chunk = kk < n ? kk : 0;
      g.est_us = g.est_us * (double)launches + 5.0 * (double)(launches - 1);
      if (!best.ok || g.est_us < best.est_us) best = g;
    }
    if (forced > 0 || k == 1) break;
  }
  return best;
}

size_t lap_workspace_bytes(const LapGeom &g) {
  return g.prog_bytes + g.yf_bytes + g.zf_bytes + g.yb_bytes + g.zb_bytes;
}
static LapRounds lap_rounds(const LapGeom &g, void *d_ws) {
  uint8_t *yb = (uint8_t *)d_ws + g.prog_bytes + g.yf_bytes + g.zf_bytes;
  return LapRounds{g.SX, g.KBY, g.YRB, g.ZRB, yb, yb + g.yb_bytes};
}
// The error word sits after the progress words of the workgroups the
// geometry was built for (NC * G; one chunk's, whatever the batch size), the
// checked kernel's monitor words 64 words further.
uint32_t *lap_err_word(const LapGeom &g, int32_t n, void *d_ws) {
  (void)n;
  return (uint32_t *)((int32_t *)d_ws + (int64_t)g.NC * g.G * LAP_PROG_STRIDE);
}

static uint32_t lap_spin_limit() {
  long v = 0;
  if (override_int("lap_spin_limit", &v)) return (uint32_t)v;  // plan override (timeout tests)
  return 1u << 22;
}
static uint32_t lap_next_epoch() {
  static std::atomic<uint32_t> ctr{(uint32_t)time(nullptr) * 2654435761u ^ (uint32_t)getpid() * 40503u};
  uint32_t e;
  do { e = ctr.fetch_add(1) + 1; } while (e == 0);
  return e;
}

typedef decltype(&lap_kernel<1, 4, true, false, false>) LapKernelFn;  // every instantiation's type
// aux: the checked kernel's monitor words (chk), or the LIT kernel's final
// 7-tuples (may be null)
// One launch of n triples on geometry g (built for n) inside the workspace
// of the allocation geometry ga (the batch's chunk geometry; g itself for a
// single launch): every region at ga's offset -- progress words, y / z rings,
// boundary rings -- and the error word / the checked kernel's monitor words at
// ga's place (lap_err_word), the same for every chunk of a batch.
static int launch_lap_fn(LapKernelFn kfn, int NW, const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                         const LapGeom &g, const LapGeom &ga, int32_t *d_scores, void *d_ws,
                         const PencilArgs &pa, const LitArgs &lit, int32_t *aux, hipStream_t stream,
                         const CheckLimits *chk) {
  if (g.lds > LDS_MAX) return TSA_EINVAL;
  if (g.prog_bytes > ga.prog_bytes || g.yf_bytes > ga.yf_bytes || g.zf_bytes > ga.zf_bytes ||
      g.yb_bytes > ga.yb_bytes || g.zb_bytes > ga.zb_bytes)
    return TSA_EINTERNAL;  // a chunk's regions must fit the batch's
  int32_t *prog = (int32_t *)d_ws;
  uint32_t *err = lap_err_word(ga, n, d_ws);
  // [max(best)] nslot, [min(best)] nslot: one slot per compute wave of this
  // launch (TSA_CHK_SLOTS), else per triple; neutral fill for waves that do not run
  int32_t *mon = chk ? (int32_t *)err + 64 : aux;
  const int64_t nslot = TSA_CHK_SLOTS ? (int64_t)g.NC * g.G * NW : (int64_t)n;
  if (chk && (hipMemsetAsync(mon, 0x80, (size_t)nslot * 4, stream) != hipSuccess ||
              hipMemsetAsync(mon + nslot, 0x7F, (size_t)nslot * 4, stream) != hipSuccess))
    return TSA_EDEVICE;
  uint8_t *yf = (uint8_t *)d_ws + ga.prog_bytes;
  uint8_t *zf = yf + ga.yf_bytes;
  uint8_t *yb = zf + ga.zf_bytes;
  const LapRounds rd{g.SX, g.KBY, g.YRB, g.ZRB, yb, yb + ga.yb_bytes};
  unsigned long long *trace = nullptr;
  char tbuf[256];  // diagnostic (override lap_trace): per-WG timestamps to a CSV file
  const char *tpath = override_str("lap_trace", tbuf, sizeof tbuf) ? tbuf : nullptr;
  const size_t tbytes = (size_t)g.blocks * LAP_TRACE_SLOTS * 8;
  if (tpath && hipMalloc(&trace, tbytes) != hipSuccess) return TSA_ENOMEM;
  if (trace && hipMemsetAsync(trace, 0, tbytes, stream) != hipSuccess)
    return TSA_EDEVICE;
  const uint32_t epoch = lap_next_epoch();
  const LapKArgs ka{d_seqs, d_offsets, g.G, g.GZ, g.NC, g.CH, g.YR, g.ZR, yf, zf, rd, prog, err,
                    d_scores, mon, pa, epoch, lap_spin_limit(), 0, g.G, yf, prog, trace, lit};
  if (launch_with_lds((const void *)kfn, g.lds, [&] {
        hipLaunchKernelGGL(kfn, dim3((uint32_t)g.grid), dim3(64 * (NW + 1)), g.lds, stream, LAP_KARGS(ka));
      }) != hipSuccess)
    return TSA_EDEVICE;
  if (chk) {
    hipLaunchKernelGGL(lap_certify, dim3((uint32_t)(TSA_CHK_SLOTS ? n : (n + 255) / 256)), dim3(256), 0, stream,
                       mon, n, nslot, (int32_t)(g.G * g.GZ * NW), *chk, d_scores);
  }
  if (hipGetLastError() != hipSuccess) return TSA_EDEVICE;
  if (trace) {
    std::vector<unsigned long long> h((size_t)g.blocks * LAP_TRACE_SLOTS);
    if (hipMemcpyAsync(h.data(), trace, h.size() * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return TSA_EDEVICE;
    (void)hipFree(trace);
    if (FILE *fp = fopen(tpath, "w")) {
      fprintf(fp, "block,tri,lap,tile,start,loop_begin,loop_end,xcc,stalls,w0_waits,loop_clk,bp_waits");
      for (int k = 8; k < 40 && k < LAP_TRACE_SLOTS; ++k)  // TSA_DIAG: wave (k-8)/4, phase (k-8)%4
        fprintf(fp, ",prof%d_%d", (k - 8) / 4, (k - 8) % 4);
      if (LAP_TRACE_SLOTS > 40) fprintf(fp, ",lag_y,lag_z");
      fprintf(fp, "\n");
      for (int64_t b = 0; b < g.blocks; ++b) {
        const unsigned long long *hb = h.data() + b * LAP_TRACE_SLOTS;
        if (hb[0] == 0) continue;  // padding block
        const int64_t slot = b >> 3, col = (slot % g.CH) * 8 + (b & 7);
        fprintf(fp, "%lld,%lld,%lld,%lld,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", (long long)b,
                (long long)(col / g.GZ), (long long)(slot / g.CH), (long long)(col % g.GZ), hb[0],
                hb[1], hb[2], hb[3], hb[4], hb[5], hb[6], hb[7]);
        for (int k = 8; k < LAP_TRACE_SLOTS; ++k) fprintf(fp, ",%llu", hb[k]);
        fprintf(fp, "\n");
      }
      fclose(fp);
    }
  }
  return TSA_OK;
}
// A batch on geometry g: one launch, or (g.chunk) launches of g.chunk
// triples one after another on the stream, each with its own epoch; the last
// chunk's geometry is built for its own size, inside g's workspace.
template <class F>
static int for_each_chunk(const LapGeom &g, int32_t n, bool f16, bool sop, bool lit, F &&launch,
                          bool ends = false) {
  const int32_t k = (g.chunk > 0 && g.chunk < n) ? g.chunk : n;
  for (int32_t c0 = 0; c0 < n; c0 += k) {
    const int32_t cn = std::min(k, n - c0);
    const LapGeom gc =
        cn == k ? g : lap_geom(cn, g.max_la, g.max_lb, g.max_lc, g.M, g.NW, false, f16, sop, lit, ends);
    if (!gc.ok && cn != k) return TSA_EINTERNAL;
    const int rc = launch(gc, c0, cn);
    if (rc) return rc;
  }
  return TSA_OK;
}
template <int M, int NW, bool F16, bool SOP>
static int launch_lap(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                      const LapGeom &g, int32_t *d_scores, void *d_ws, const PencilArgs &pa,
                      hipStream_t stream, const CheckLimits *chk) {
  if (chk && F16) return TSA_EINVAL;
  // pa.lam != 0: the V-space cell (make_args(..., vs = true); f16 only)
  LapKernelFn kfn = chk ? lap_kernel<M, NW, F16, SOP, !F16> : lap_kernel<M, NW, F16, SOP, false>;
  if constexpr (F16) {
    if (pa.lam != 0) kfn = lap_kernel<M, NW, true, SOP, false, false, false, true>;
  }
  return for_each_chunk(g, n, F16, SOP, false, [&](const LapGeom &gc, int32_t c0, int32_t cn) {
    return launch_lap_fn(kfn, NW, d_seqs, d_offsets + 3 * (int64_t)c0, cn, gc, g, d_scores + c0, d_ws, pa,
                         LitArgs{}, nullptr, stream, chk);
  });
}
template <int M, int NW, bool SOP>
static int launch_lap_lit(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, const LapGeom &g,
                          int32_t *d_scores, int32_t *d_final7, void *d_ws, const PencilArgs &pa,
                          const LitArgs &lit, hipStream_t stream) {
  return for_each_chunk(g, n, false, SOP, true, [&](const LapGeom &gc, int32_t c0, int32_t cn) {
    return launch_lap_fn(lap_kernel<M, NW, false, SOP, false, false, true>, NW, d_seqs, d_offsets + 3 * (int64_t)c0,
                         cn, gc, g, d_scores + c0, d_ws, pa, lit, d_final7 ? d_final7 + 7 * (int64_t)c0 : nullptr,
                         stream, nullptr);
  });
}

int lap_launch_lit(const LapGeom &g, bool sop, const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                   int32_t *d_scores, int32_t *d_final7, void *d_ws, const KParams &kp, hipStream_t stream,
                   int32_t **d_err) {
  if (g.M > 2 || (g.NW != 4 && g.NW != 8)) return TSA_EINVAL;
  if (d_err) {  // synchronous caller: clear the error word, it reads it back
    *d_err = (int32_t *)lap_err_word(g, n, d_ws);
    if (hipMemsetAsync(*d_err, 0, sizeof(int32_t), stream) != hipSuccess) return TSA_EDEVICE;
  }
  PencilArgs pa{};  // the literal form reads only the packed flag; zero faces
  pa.packed = kp.packed;
  const LitArgs lit = lit_args(kp);
  return TSA_LIT_SHAPES(launch_lap_lit, g.M, g.NW, sop, d_seqs, d_offsets, n, g, d_scores, d_final7, d_ws, pa,
                        lit, stream);
}

int lap_launch(const LapGeom &g, bool f16, bool sop, const uint8_t *d_seqs,
               const int64_t *d_offsets, int32_t n, int32_t *d_scores, void *d_ws,
               const PencilArgs &pa, hipStream_t stream, int32_t **d_err,
               const CheckLimits *chk) {
  if (d_err) {  // synchronous caller: clear the error word, it reads it back
    *d_err = (int32_t *)lap_err_word(g, n, d_ws);
    if (hipMemsetAsync(*d_err, 0, sizeof(int32_t), stream) != hipSuccess) return TSA_EDEVICE;
  }
  return TSA_LAP_SHAPES(launch_lap, g.M, g.NW, f16, sop, d_seqs, d_offsets, n, g, d_scores, d_ws,
                        pa, stream, chk);
}

// ---------------------------------------------------------------------------
// The end search (tsa_score_batch_ends_lap): lap_ends_kernel on a geometry from
// lap_geom(..., ends = true), then lap_ends_reduce. The workspace is the
// checked kernel's (monitor slots included) with the key slots behind it, 8
// bytes per compute wave of every logical workgroup of a launch.
size_t lap_ends_workspace_bytes(const LapGeom &g) {
  const size_t keys = (size_t)g.NC * g.G * g.NW * sizeof(unsigned long long);
  return lap_workspace_bytes(g) + ((keys + 255) & ~(size_t)255);
}
typedef decltype(&lap_ends_kernel<1, 4, false>) LapEndsKernelFn;  // every instantiation's type
// One launch of n triples on geometry g inside the workspace of the batch's
// geometry ga (as launch_lap_fn). The monitor and key slots get their neutral
// fill here, so the workspace may hold anything.
static int launch_lap_ends_fn(LapEndsKernelFn kfn, int NW, const uint8_t *d_seqs, const int64_t *d_offsets,
                              int32_t n, const LapGeom &g, const LapGeom &ga, int32_t *d_scores, int32_t *d_ends,
                              void *d_ws, const PencilArgs &pa, hipStream_t stream, const CheckLimits &lim) {
  if (g.lds > LDS_MAX) return TSA_EINVAL;
  if (g.prog_bytes > ga.prog_bytes || g.yf_bytes > ga.yf_bytes || g.zf_bytes > ga.zf_bytes ||
      g.yb_bytes > ga.yb_bytes || g.zb_bytes > ga.zb_bytes || (int64_t)g.NC * g.G > (int64_t)ga.NC * ga.G)
    return TSA_EINTERNAL;  // a chunk's regions must fit the batch's
  int32_t *prog = (int32_t *)d_ws;
  uint32_t *err = lap_err_word(ga, n, d_ws);
  int32_t *mon = (int32_t *)err + 64;
  unsigned long long *ekey = (unsigned long long *)((uint8_t *)d_ws + lap_workspace_bytes(ga));
  const int64_t nslot = (int64_t)g.NC * g.G * NW;
  if (hipMemsetAsync(mon, 0x80, (size_t)nslot * 4, stream) != hipSuccess ||
      hipMemsetAsync(mon + nslot, 0x7F, (size_t)nslot * 4, stream) != hipSuccess ||
      hipMemsetAsync(ekey, 0, (size_t)nslot * 8, stream) != hipSuccess)
    return TSA_EDEVICE;
  uint8_t *yf = (uint8_t *)d_ws + ga.prog_bytes;
  uint8_t *zf = yf + ga.yf_bytes;
  uint8_t *yb = zf + ga.zf_bytes;
  const LapRounds rd{g.SX, g.KBY, g.YRB, g.ZRB, yb, yb + ga.yb_bytes};
  const uint32_t epoch = lap_next_epoch();
  const LapKArgs ka{d_seqs, d_offsets, g.G, g.GZ, g.NC, g.CH, g.YR, g.ZR, yf, zf, rd, prog, err,
                    d_scores, mon, pa, epoch, lap_spin_limit(), 0, g.G, yf, prog, nullptr, LitArgs{}};
  if (launch_with_lds((const void *)kfn, g.lds, [&] {
        hipLaunchKernelGGL(kfn, dim3((uint32_t)g.grid), dim3(64 * (NW + 1)), g.lds, stream, LAP_KARGS(ka), ekey);
      }) != hipSuccess)
    return TSA_EDEVICE;
  hipLaunchKernelGGL(lap_ends_reduce, dim3((uint32_t)n), dim3(256), 0, stream, mon, ekey, nslot,
                     (int32_t)(g.G * g.GZ * NW), lim, err, epoch, d_scores, d_ends);
  return hipGetLastError() == hipSuccess ? TSA_OK : TSA_EDEVICE;
}
template <int M, int NW, bool SOP>
static int launch_lap_ends(const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n, const LapGeom &g,
                           int32_t *d_scores, int32_t *d_ends, void *d_ws, const PencilArgs &pa,
                           hipStream_t stream, const CheckLimits &lim) {
  return for_each_chunk(
      g, n, false, SOP, false,
      [&](const LapGeom &gc, int32_t c0, int32_t cn) {
        return launch_lap_ends_fn(lap_ends_kernel<M, NW, SOP>, NW, d_seqs, d_offsets + 3 * (int64_t)c0, cn, gc, g,
                                  d_scores + c0, d_ends + 3 * (int64_t)c0, d_ws, pa, stream, lim);
      },
      true);
}

int lap_launch_ends(const LapGeom &g, bool sop, const uint8_t *d_seqs, const int64_t *d_offsets, int32_t n,
                    int32_t *d_scores, int32_t *d_ends, void *d_ws, const PencilArgs &pa, hipStream_t stream,
                    int32_t **d_err, const CheckLimits *chk) {
  if (g.M > 2 || (g.NW != 4 && g.NW != 8) || g.max_la - 1 > LAP_END_XMAX) return TSA_EINVAL;
  if (d_err) {  // synchronous caller: clear the error word, it reads it back
    *d_err = (int32_t *)lap_err_word(g, n, d_ws);
    if (hipMemsetAsync(*d_err, 0, sizeof(int32_t), stream) != hipSuccess) return TSA_EDEVICE;
  }
  const CheckLimits lim = chk ? *chk : CheckLimits{INT32_MAX, INT32_MIN};  // exact a priori: nothing to certify
  return TSA_LIT_SHAPES(launch_lap_ends, g.M, g.NW, sop, d_seqs, d_offsets, n, g, d_scores, d_ends, d_ws, pa, stream,
                        lim);
}

// ---------------------------------------------------------------------------
// One cube split over devices by laps (tsa_score_gpu_multi): part p runs laps
// [L0_p, L1_p) on its own device; part p's last lap writes its y records into
// part p+1's workspace and part p+1's first lap copies its progress words into
// part p's, so each hand-off crossing the link is a posted store and every
// poll stays local. The error word and the score live with the last part.
static int launch_split_fn(LapKernelFn kfn, int NW, const LapGeom &g, const PencilArgs &pa, const LitArgs &lit,
                           const LapPart *parts, int np, int32_t *d_score, uint32_t *d_err) {
  const uint32_t epoch = lap_next_epoch();
  const uint32_t spin = lap_spin_limit();
  for (int p = 0; p < np; ++p) {
    const LapPart &q = parts[p];
    if (hipSetDevice(q.device) != hipSuccess) return TSA_EDEVICE;
    int32_t *prog = (int32_t *)q.d_ws;
    uint8_t *yf = (uint8_t *)q.d_ws + g.prog_bytes;
    uint8_t *zf = yf + g.yf_bytes;
    uint8_t *yf_out = p + 1 < np ? (uint8_t *)parts[p + 1].d_ws + g.prog_bytes : yf;
    int32_t *prog_in = p > 0 ? (int32_t *)parts[p - 1].d_ws : prog;
    const int64_t blocks = (int64_t)(q.L1 - q.L0) * g.CH * 8;
    const LapKArgs ka{q.d_seqs, q.d_offsets, g.G, g.GZ, g.NC, g.CH, g.YR, g.ZR, yf, zf, lap_rounds(g, q.d_ws),
                      prog, d_err, d_score, (int32_t *)nullptr, pa, epoch, spin, q.L0, q.L1, yf_out, prog_in,
                      (unsigned long long *)nullptr, lit};
    if (launch_with_lds((const void *)kfn, g.lds, [&] {
          hipLaunchKernelGGL(kfn, dim3((uint32_t)blocks), dim3(64 * (NW + 1)), g.lds, q.stream, LAP_KARGS(ka));
        }) != hipSuccess)
      return TSA_EDEVICE;
  }
  return TSA_OK;
}
template <int M, int NW, bool F16, bool SOP>
static int launch_lap_split(const LapGeom &g, const PencilArgs &pa, const LapPart *parts, int np,
                            int32_t *d_score, uint32_t *d_err) {
  return launch_split_fn(lap_kernel<M, NW, F16, SOP, false, true>, NW, g, pa, LitArgs{}, parts, np, d_score, d_err);
}
template <int M, int NW, bool SOP>
static int launch_lap_split_lit(const LapGeom &g, const PencilArgs &pa, const LitArgs &lit, const LapPart *parts,
                                int np, int32_t *d_score, uint32_t *d_err) {
  return launch_split_fn(lap_kernel<M, NW, false, SOP, false, true, true>, NW, g, pa, lit, parts, np, d_score,
                         d_err);
}
static int split_parts_ok(const LapGeom &g, const LapPart *parts, int np) {
  if (np < 1 || g.lds > LDS_MAX) return 0;
  for (int p = 0; p < np; ++p)
    if (parts[p].L0 >= parts[p].L1 || parts[p].L0 != (p ? parts[p - 1].L1 : 0)) return 0;
  return parts[np - 1].L1 == g.G;
}

int lap_launch_split(const LapGeom &g, bool f16, bool sop, const PencilArgs &pa, const LapPart *parts,
                     int np, int32_t *d_score, uint32_t *d_err) {
  if (!split_parts_ok(g, parts, np)) return TSA_EINVAL;
  return TSA_LAP_SHAPES(launch_lap_split, g.M, g.NW, f16, sop, g, pa, parts, np, d_score, d_err);
}

int lap_launch_split_lit(const LapGeom &g, bool sop, const KParams &kp, const LapPart *parts, int np,
                         int32_t *d_score, uint32_t *d_err) {
  if (!split_parts_ok(g, parts, np) || g.M > 2 || (g.NW != 4 && g.NW != 8)) return TSA_EINVAL;
  PencilArgs pa{};  // as lap_launch_lit: the packed flag only, zero faces
  pa.packed = kp.packed;
  const LitArgs lit = lit_args(kp);
  return TSA_LIT_SHAPES(launch_lap_split_lit, g.M, g.NW, sop, g, pa, lit, parts, np, d_score, d_err);
}

}  // namespace tsa
