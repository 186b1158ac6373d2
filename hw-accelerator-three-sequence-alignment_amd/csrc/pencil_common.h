// pencil_common.h -- device helpers and packed constants shared
// by the register-systolic kernels: the batch helix (pencil_kernel.hip) and the
// single-cube lap kernel (lap_kernel.hip). See pencil_kernel.hip for the design.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#include "pencil_kernel.h"

namespace tsa {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

constexpr size_t LDS_MAX = 160 * 1024;
constexpr int REC_BYTES = 16;      // {Iy, Ixy, Iyz, best} packed pairs per lane

// Packed (both halves) constants. int16 form: two's complement; exact-f16 form
// (helix kernel, F16): f16 bits, pair penalties and f_pair with the mismatch
// folded in, h_* the 2^13-scaled score deltas and h_c3 the triple-score base.
struct PencilArgs {
  uint32_t E, O, E2, OE, O2;    // packed penalties GE, GO, 2GE, GO+GE, 2GO
  uint32_t f_single, f_pair;    // face messages of an all-zero cell
  uint32_t dm, mm;              // match-mismatch, mismatch
  uint32_t s3_d1, s3_d0, s3_ne; // RTL: s3 = ne + eab*(d0 + ebc*d1)
  uint32_t h_dm, h_c3;           // 2^13 (match-mismatch); RTL ne
  uint32_t h_sbc, h_k0, h_kd;     // per-row registers, see cell_messages_f16
  float dmf;                      // match - mismatch (per-position DMC, exact f16)
  int32_t sop;                  // TSA_S3_SOP
  int32_t packed;               // 2-bit packed input symbols (tsa_sym)
  // V-space helix (cell_messages_vs): values of cell (x,y,z) shifted by
  // lam*(x+y+z); lam = GE = -MISMATCH, f16 bits in both halves
  int32_t lam;                  // lam as an integer (0: not V-space)
  uint32_t v_lam, v_cP, v_dO;   // lam, GO + MISMATCH + lam, GO - GE
  float d0f, d1f;               // RTL s3 deltas (V-space K = (d0 + [b=c] d1) / code(b))
  // Integer-pattern V-space cell (cell_messages_vi): a half holds u = bias + 8 V
  int32_t bias;                 // 0: the float cell
  uint32_t i_bias;              // bias in both halves
  uint32_t i_lam, i_cP, i_dO;   // 8 lam, 8 (GO + MISMATCH + lam), 8 (GO - GE): both halves, 32-bit subtrahends
  int32_t dm8, d0_8, d1_8;      // 8 (match - mismatch), 8 d0, 8 d1 (weights 8 w / code)
  // End search (the END instantiations, end_class): candidates on the end faces only
  int32_t end_face;
};

// Literal RTL arithmetic (literal_kernel.hip, the lap kernel's LIT form):
// constants as int16 values shifted left by sh = 16 - SCORE_BITS, both halves,
// so packed u16 adds wrap exactly at the RTL word.
struct LitArgs {
  uint32_t n2E, nOE, n2O;   // -2GE, -(GO+GE), -2GO
  uint32_t dmS, mmE, nDOE;  // match - mismatch, mismatch - GE, -(GO - GE)
  uint32_t d1S, d0S, neS;   // RTL s3 = ne + [a=b](d0 + [b=c] d1)
  uint32_t mm3S;            // SOP s3 = 3 mismatch + dm ([a=b] + [b=c] + [a=c])
  // pushes of a zero cell (the faces): to Ix / Iy / Iz, to a pair target with
  // its pair score a match (1) or not (0), to M by the successor's indicators
  uint32_t fS[3], fP[2], fM[8];
  int32_t sh, packed;
  int32_t end_face;         // end search (literal_kernel END): candidates on the end faces only
};
LitArgs lit_args(const KParams &kp);

// positions per lane: M packed pairs cover LC <= 128*M (1, 2, 4 or 8)
static inline int32_t pencil_pairs(int32_t max_lc) {
  return max_lc <= 128 ? 1 : max_lc <= 256 ? 2 : max_lc <= 512 ? 4 : 8;
}

// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a),
                                                                __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
// v_pk_mad_u16 / v_pk_min_u16 written as asm: left to itself hipcc rewrites
// min(x,1)*d+c into per-half compares and selects (6 ops instead of 2).
__device__ __forceinline__ uint32_t pk_mad(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// per-half (a & b) != 0 -> 1 / 0 (one-hot symbols). `ones` = 0x00010001 in a
// VGPR: a VOP3P inline constant would feed 0 to the high half.
__device__ __forceinline__ uint32_t pk_eq1(uint32_t a, uint32_t b, uint32_t ones) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a & b), "v"(ones));
  return r;
}
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) {
  return (mask & a) | (~mask & b);
}
// one v_bfi_b32 (hipcc otherwise splits a group of bfi's with a shared mask
// into v_not + v_and + v_and_or)
__device__ __forceinline__ uint32_t vbfi(uint32_t mask, uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
  return r;
}
// One LDS-DMA of 16 B per lane: LDS[m0 + lane*16] <- *gsrc (sc1: bypass L1).
// Issued from inline asm so that hipcc does not treat it as an in-flight LDS
// write and drain vmcnt(0) before every ds_read of the step loop; the
// consumer waits for it with an explicit counted s_waitcnt vmcnt
// (cdna_hip_programming.md 5.7: M0 must be set in the same statement).
__device__ __forceinline__ void dma16(const void *gsrc, const void *lds_dst) {
  unsigned keep;
  const unsigned dst = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)lds_dst;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off sc1\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(dst))
      : "memory");
}
// 4-byte LDS-DMA from lane 0 only (the caller guards with lane == 0).
__device__ __forceinline__ void dma4(const void *gsrc, const void *lds_dst) {
  unsigned keep;
  const unsigned dst = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)lds_dst;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, off sc1\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(dst))
      : "memory");
}
// 16-byte LDS record read as one ds_read_b128 (lane-contiguous, conflict
// free). Through a generic pointer hipcc splits it into two ds_read2_b32
// with a 16 B lane stride, a 4-way bank conflict (SQ_LDS_BANK_CONFLICT).
typedef unsigned u32x4_lds __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 lds_read16(const uint8_t *p) {
  const __attribute__((address_space(3))) u32x4_lds *q =
      (const __attribute__((address_space(3))) u32x4_lds *)(const __attribute__((address_space(3))) void *)p;
  const u32x4_lds v = *q;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void lds_write16(uint8_t *p, uint4 v) {
  __attribute__((address_space(3))) u32x4_lds *q =
      (__attribute__((address_space(3))) u32x4_lds *)(__attribute__((address_space(3))) void *)p;
  *q = (u32x4_lds){v.x, v.y, v.z, v.w};
}
// The same through an LDS base pointer plus a byte offset: a compile-time
// offset folds into the ds instruction's offset field (no VALU address add)
typedef __attribute__((address_space(3))) uint8_t lds_u8;
__device__ __forceinline__ lds_u8 *to_lds(uint8_t *p) {
  return (lds_u8 *)(__attribute__((address_space(3))) void *)p;
}
__device__ __forceinline__ uint4 lds_read16_at(const lds_u8 *base, int off) {
  const u32x4_lds v = *(const __attribute__((address_space(3))) u32x4_lds *)(base + off);
  return make_uint4(v.x, v.y, v.z, v.w);
}
// 8 bytes of a record as one ds_read_b64
__device__ __forceinline__ uint2 lds_read8_at(const lds_u8 *base, int off) {
  const uint64_t v = *(const __attribute__((address_space(3))) uint64_t *)(base + off);
  return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
__device__ __forceinline__ void lds_write16_at(lds_u8 *base, int off, uint4 v) {
  *(__attribute__((address_space(3))) u32x4_lds *)(base + off) = (u32x4_lds){v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint32_t ror1(uint32_t v) {  // lane l <- lane l-1, lane 0 <- lane 63
  // mov_dpp (old = undef): wave_ror:1 reads a valid lane for every lane
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x13C, 0xF, 0xF, false);
}

// One step of M packed cell pairs: scores (src/PE_1cyc.v:159-162) on one-hot
// symbols, the 7 states, and the 7 outgoing messages max_s(S[s] - P[T][s])
// (src/PE_1cyc.v:164-218) grouped by equal penalty; oBest = MAX7 of the states.
template <int M, int SOPM = -1>  // SOPM: 0 RTL, 1 SOP, -1 read pa.sop
__device__ __forceinline__ void cell_messages(
    const uint32_t (&a)[M], const uint32_t (&b)[M], const uint32_t (&c)[M], uint32_t ones,
    const PencilArgs &pa, const uint32_t (&inIx)[M], const uint32_t (&inIy)[M],
    const uint32_t (&inIz)[M], const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M],
    const uint32_t (&inIxz)[M], const uint32_t (&inM)[M], uint32_t (&nIx)[M], uint32_t (&oIy)[M],
    uint32_t (&oIz)[M], uint32_t (&oIxy)[M], uint32_t (&oIyz)[M], uint32_t (&oIxz)[M],
    uint32_t (&oBest)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const uint32_t eab = pk_eq1(a[i], b[i], ones);
    const uint32_t eac = pk_eq1(a[i], c[i], ones);
    const uint32_t ebc = pk_eq1(b[i], c[i], ones);
    const uint32_t s2ab = pk_mad(eab, pa.dm, pa.mm);
    const uint32_t s2ac = pk_mad(eac, pa.dm, pa.mm);
    const uint32_t s2bc = pk_mad(ebc, pa.dm, pa.mm);
    uint32_t s3;
    if (SOPM < 0 ? pa.sop != 0 : SOPM == 1) s3 = pk_add(pk_add(s2ab, s2bc), s2ac);
    else s3 = pk_mad(eab, pk_mad(ebc, pa.s3_d1, pa.s3_d0), pa.s3_ne);
    const uint32_t sM = pk_add(inM[i], s3);
    const uint32_t sX = inIx[i], sY = inIy[i], sZ = inIz[i];
    const uint32_t sXY = pk_add(inIxy[i], s2ab);
    const uint32_t sYZ = pk_add(inIyz[i], s2bc);
    const uint32_t sXZ = pk_add(inIxz[i], s2ac);
    // two-input maxes only (no packed int16 max3): pairs shared between groups
    const uint32_t pYZ = pk_max(sY, sZ), pXZ = pk_max(sX, sZ), pXY = pk_max(sX, sY);
    const uint32_t qXY_XZ = pk_max(sXY, sXZ), qXY_YZ = pk_max(sXY, sYZ), qYZ_XZ = pk_max(sYZ, sXZ);
    const uint32_t A1 = pk_max(pYZ, qXY_XZ);  // Ix  <- {Iy,Iz,Ixy,Ixz} at GO+GE
    const uint32_t A2 = pk_max(pXZ, qXY_YZ);  // Iy  <- {Ix,Iz,Ixy,Iyz}
    const uint32_t A3 = pk_max(pXY, qYZ_XZ);  // Iz  <- {Ix,Iy,Iyz,Ixz}
    const uint32_t C1 = pk_max(pXY, sXY);     // Ixy <- {Ix,Iy,Ixy} at GE
    const uint32_t C2 = pk_max(pYZ, sYZ);     // Iyz <- {Iy,Iz,Iyz}
    const uint32_t C3 = pk_max(pXZ, sXZ);     // Ixz <- {Ix,Iz,Ixz}
    // GO >= GE: the highest-penalty group of every target may be widened to
    // all 7 states (see cell_messages_f16), so it is the MAX7 minus one penalty
    const uint32_t best = pk_max(pk_max(A1, A2), sM);  // A1 | A2 = the six gap states
    const uint32_t bO = pk_sub(best, pa.O), bO2 = pk_sub(best, pa.O2);
    oBest[i] = best;
    nIx[i] = pk_max(pk_max(pk_sub(sX, pa.E2), pk_sub(A1, pa.OE)), bO2);
    oIy[i] = pk_max(pk_max(pk_sub(sY, pa.E2), pk_sub(A2, pa.OE)), bO2);
    oIz[i] = pk_max(pk_max(pk_sub(sZ, pa.E2), pk_sub(A3, pa.OE)), bO2);
    oIxy[i] = pk_max(pk_sub(C1, pa.E), bO);
    oIyz[i] = pk_max(pk_sub(C2, pa.E), bO);
    oIxz[i] = pk_max(pk_sub(C3, pa.E), bO);
  }
}

// The pk_mad operands must be VGPRs (inline asm "v"): pin them once, or hipcc
// re-materialises them from SGPRs with a v_mov before every use.
__device__ __forceinline__ PencilArgs pin_score_consts(const PencilArgs &pa) {
  PencilArgs r = pa;
  asm volatile("" : "+v"(r.dm), "+v"(r.mm), "+v"(r.s3_d1), "+v"(r.s3_d0), "+v"(r.s3_ne));
  return r;
}

// ---------------------------------------------------------------------------
// Exact-f16 arithmetic for the helix kernel. Every DP value is an integer; when
// the host proves all of them (and every candidate) lie in [-2048, 2048]
// (trialign_api.hip:pencil_exact), IEEE f16 add/fma/maximum on them are exact,
// and CDNA4's v_pk_maximum3_f16 folds two packed maxes into one instruction.
// Symbol codes are one-hot at bits 11..14 (0x800 << s), so min_u16(a & b, 0x800)
// is 0x0800 = f16 2^-13 on a match and 0 otherwise; the match-mismatch deltas
// are pre-scaled by 2^13 so a single v_pk_fma_f16 adds a pair score. The
// mismatch score of each pair target is folded into the penalties its
// messages carry (Ep = GE - mismatch, Op = GO - mismatch, and f_pair).
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2 H(uint32_t v) { return __builtin_bit_cast(h2, v); }
__device__ __forceinline__ uint32_t U(h2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ h2 hmax(h2 a, h2 b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ h2 hmax3(h2 a, h2 b, h2 c) { return hmax(hmax(a, b), c); }
// The messages' maxes: the compiler fuses each into one v_pk_maximum3_f16 where
// the callers keep the inner pairs distinct (the instruction written as asm
// measured slower: the asm blocks constrain the scheduler more than they save)
__device__ __forceinline__ h2 vmax3(h2 a, h2 b, h2 c) { return hmax3(a, b, c); }
__device__ __forceinline__ h2 hfma(h2 a, h2 b, h2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ uint32_t umin2(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a),
                                                                 __builtin_bit_cast(us2, b)));
}
constexpr uint32_t SYM0 = 0x800u;  // helix symbol codes: SYM0 << s
// Per half: f16(dm / f16value(code)) for a one-hot code (a power of two:
// 2^-13, 2^-11, 2^-7 or 2), 0 for code 0 (padding); exact for |dm| <= 7.
__device__ __forceinline__ uint32_t dm_over_code(float dm, uint32_t codes) {
  uint32_t r = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint16_t c = (uint16_t)(codes >> (16 * h));
    if (c != 0) {
      const _Float16 v = (_Float16)(dm / (float)__builtin_bit_cast(_Float16, c));
      r |= (uint32_t)__builtin_bit_cast(uint16_t, v) << (16 * h);
    }
  }
  return r;
}

// Terms that depend only on (b, c) are per-position constants for a whole row
// (b changes when a position starts a new row at x = 1), kept in registers:
//   SBC = dm*[b=c]                       (f16) added to the Iyz input
//   K   = RTL: 2^13 (d0 + d1*[b=c])      fma multiplier of [a=b] for M
//         SOP: 3 mismatch + dm*[b=c]     added to the M input
template <int M, bool SOP>
__device__ __forceinline__ void cell_messages_f16(
    const uint32_t (&a)[M], const uint32_t (&b)[M], const uint32_t (&c)[M],
    const uint32_t (&SBC)[M], const uint32_t (&K)[M], const uint32_t (&DMC)[M], uint32_t Q,
    const PencilArgs &pa,
    const uint32_t (&inIx)[M], const uint32_t (&inIy)[M], const uint32_t (&inIz)[M],
    const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M], const uint32_t (&inIxz)[M],
    const uint32_t (&inM)[M], uint32_t (&nIx)[M], uint32_t (&oIy)[M], uint32_t (&oIz)[M],
    uint32_t (&oIxy)[M], uint32_t (&oIyz)[M], uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
  const h2 DM = H(pa.h_dm), E = H(pa.E), O = H(pa.O), E2 = H(pa.E2), OE = H(pa.OE), O2 = H(pa.O2);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    // a & c is c's code (a power of two) on a match, 0 otherwise, and
    // DMC = (match - mismatch) / code(c) per position: the product is exact
    const h2 eab = H(umin2(a[i] & b[i], Q)), eac = H(a[i] & c[i]);
    const h2 DMCi = H(DMC[i]);
    const h2 sXY = hfma(eab, DM, H(inIxy[i]));  // src/PE_1cyc.v:159-161 (+mismatch folded)
    const h2 sXZ = hfma(eac, DMCi, H(inIxz[i]));
    const h2 sYZ = H(inIyz[i]) + H(SBC[i]);
    h2 sM;                                       // src/PE_1cyc.v:162
    if constexpr (SOP) sM = hfma(eab, DM, hfma(eac, DMCi, H(inM[i]))) + H(K[i]);
    else sM = hfma(eab, H(K[i]), H(inM[i])) + H(pa.h_c3);  // ne + [a=b](d0 + [b=c] d1)
    const h2 sX = H(inIx[i]), sY = H(inIy[i]), sZ = H(inIz[i]);
    // With GO >= GE (pencil_supported) a penalty group may take in any state
    // that already reaches the target at a penalty no larger (2GE <= GO+GE <=
    // 2GO, GE <= GO): each single target's GO+GE group takes in the target's
    // own state, so the three share max(Ix,Iy,Iz); each target's highest
    // group ({M,Iyz} at 2GO for Ix, {M,Iz,Iyz,Ixz} at GO for Ixy, ...) takes in
    // all 7, so it is MAX7 - penalty, shared by all six gap targets.
    // vmax3(a, b, c) = max(max(a, b), c): the inner pairs are all distinct, so
    // the compiler cannot CSE one and fuses every pair into one max3
    const h2 S3 = vmax3(sX, sY, sZ);
    const h2 A1 = vmax3(S3, sXY, sXZ);   // Ix  <- {Iy,Iz,Ixy,Ixz} (+Ix) at GO+GE
    const h2 A2 = vmax3(S3, sYZ, sXY);   // Iy  <- {Ix,Iz,Ixy,Iyz} (+Iy)
    const h2 A3 = vmax3(sYZ, sXZ, S3);   // Iz  <- {Ix,Iy,Iyz,Ixz} (+Iz)
    const h2 C1 = vmax3(sX, sXY, sY);    // Ixy <- {Ix,Iy,Ixy} at GE
    const h2 C2 = vmax3(sY, sYZ, sZ);
    const h2 C3 = vmax3(sZ, sXZ, sX);
    const h2 best = vmax3(A1, sYZ, sM);  // A1 | Iyz = the six gap states
    const h2 bO = best - O, bO2 = best - O2;
    oBest[i] = U(best);
    nIx[i] = U(vmax3(sX - E2, A1 - OE, bO2));
    oIy[i] = U(vmax3(sY - E2, A2 - OE, bO2));
    oIz[i] = U(vmax3(sZ - E2, A3 - OE, bO2));
    oIxy[i] = U(vmax3(C1 - E, bO, bO));
    oIyz[i] = U(vmax3(C2 - E, bO, bO));
    oIxz[i] = U(vmax3(C3 - E, bO, bO));
  }
}

// The same cell in V-space (tests/test_cell_algebra.py replays it against the
// oracle): every value of cell (x,y,z) is stored shifted by lam*(x+y+z), a
// potential -- every path into a cell gains the same amount, so no max
// changes -- with lam = GE = -MISMATCH (the RTL's constants: 1). A transition
// that advances x+y+z by d then pays lam*d less, so (f16 form, the mismatch
// folded into the pair messages as above):
//  * the pair targets' extend penalty GE - MISMATCH - 2 lam vanishes:
//      Ixy' = max(G_z, best - (GO - GE)),  G_z = max(Ix, Iy, Ixy)  (G_x, G_y alike);
//  * a single target is the better of its own extension and the two pair
//    messages that share its gaps (the penalty table is a sum over the gapped
//    axes, src/PE_1cyc.v:172-194, so max(Ixy', Ixz') covers every other source):
//      Ix' = max(Ix - lam, max(Ixy', Ixz') - (GO + MISMATCH + lam));
//  * M adds no constant: 3 MISMATCH + 3 lam = 0 (the SOP form folds 3 lam into K).
// 24 instructions per pair (RTL) against cell_messages_f16's 33. Zero faces
// become lam*q at coordinate sum q: the kernel injects those (pencil_kernel.hip).
template <int M, bool SOP>
__device__ __forceinline__ void cell_messages_vs(
    const uint32_t (&a)[M], const uint32_t (&b)[M], const uint32_t (&c)[M],
    const uint32_t (&SBC)[M], const uint32_t (&K)[M], const uint32_t (&DMC)[M], const uint32_t (&DMB)[M],
    const PencilArgs &pa,
    const uint32_t (&inIx)[M], const uint32_t (&inIy)[M], const uint32_t (&inIz)[M],
    const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M], const uint32_t (&inIxz)[M],
    const uint32_t (&inM)[M], uint32_t (&nIx)[M], uint32_t (&oIy)[M], uint32_t (&oIz)[M],
    uint32_t (&oIxy)[M], uint32_t (&oIyz)[M], uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
  const h2 LAM = H(pa.v_lam), CP = H(pa.v_cP), DO = H(pa.v_dO);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    // a & b is b's code on a match, 0 otherwise; DMB = dm / code(b) and (RTL) K
    // = (d0 + [b=c] d1) / code(b) per position and row: the products are exact
    const h2 eab = H(a[i] & b[i]), eac = H(a[i] & c[i]), DMCi = H(DMC[i]), DMBi = H(DMB[i]);
    const h2 sXY = hfma(eab, DMBi, H(inIxy[i]));  // src/PE_1cyc.v:159-161 (+mismatch folded)
    const h2 sXZ = hfma(eac, DMCi, H(inIxz[i]));
    const h2 sYZ = H(inIyz[i]) + H(SBC[i]);
    h2 sM;                                       // src/PE_1cyc.v:162
    if constexpr (SOP) sM = hfma(eab, DMBi, hfma(eac, DMCi, H(inM[i]))) + H(K[i]);
    else sM = hfma(eab, H(K[i]), H(inM[i]));     // ne + 3 lam = 0
    const h2 sX = H(inIx[i]), sY = H(inIy[i]), sZ = H(inIz[i]);
    const h2 Gx = vmax3(sY, sZ, sYZ), Gy = vmax3(sX, sZ, sXZ), Gz = vmax3(sX, sY, sXY);
    const h2 best = vmax3(Gx, Gy, hmax(sXY, sM));
    const h2 b1 = best - DO;
    const h2 pXY = hmax(Gz, b1), pYZ = hmax(Gx, b1), pXZ = hmax(Gy, b1);
    const h2 qXY = pXY - CP, qYZ = pYZ - CP, qXZ = pXZ - CP;
    oBest[i] = U(best);
    oIxy[i] = U(pXY);
    oIyz[i] = U(pYZ);
    oIxz[i] = U(pXZ);
    nIx[i] = U(vmax3(sX - LAM, qXY, qXZ));
    oIy[i] = U(vmax3(sY - LAM, qXY, qYZ));
    oIz[i] = U(vmax3(sZ - LAM, qYZ, qXZ));
  }
}

// The V-space cell on integer bit patterns (tests/test_cell_int_algebra.py
// replays it on packed words against the oracle). A half holds the unsigned
// u = bias + 8 V, kept inside [0x0400, 0x7BFF] by the host (pencil_kernel.hip:
// use_vi): a positive, normal, finite f16 pattern, for which IEEE order is the
// unsigned integer order, so every max stays a v_pk_maximum3_f16 and returns the
// bitwise maximum exactly. What the float cell adds as packed f16 -- SBC, the
// three - CP, the three - LAM, - DO: constants and per-row registers, never two
// DP values -- is one 32-bit integer add or subtract of the packed constant
// (c_hi * 65536 + c_lo, formed in signed arithmetic): both halves come out right
// while each half's true result lies in [0, 65535], which the window gives.
// v_add_u32 / v_sub_u32 issue in 2 cycles where every packed op takes 4
// (tools/valu_peak.hip, profiles/r9_valu_mix.jsonl). Symbol codes are one-hot
// 1, 2, 4, 8, so a & b is b's code on a match, and the per-row weights DMB =
// 8 dm / code(b), DMC = 8 dm / code(c), K = 8 (d0 + [b=c] d1) / code(b) are
// integers (per half, mod 2^16): v_pk_mad_u16 adds a bonus with no carry
// between the halves. The same 24 operations per register as cell_messages_vs.
__device__ __forceinline__ uint32_t imax(uint32_t a, uint32_t b) { return U(hmax(H(a), H(b))); }
__device__ __forceinline__ uint32_t imax3(uint32_t a, uint32_t b, uint32_t c) {
  return U(vmax3(H(a), H(b), H(c)));
}
// Per half: (w8 / code) mod 2^16 for a one-hot code 1, 2, 4 or 8 (w8 a multiple
// of 8), 0 for code 0 (padding).
__device__ __forceinline__ uint32_t w8_over_code(int32_t w8, uint32_t codes) {
  uint32_t r = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int32_t c = (int32_t)((codes >> (16 * h)) & 0xFFFFu);
    if (c != 0) r |= ((uint32_t)(w8 / c) & 0xFFFFu) << (16 * h);
  }
  return r;
}
// Two 16-bit two's-complement halves -> the word a 32-bit add needs to add both
// (hi * 65536 + lo in signed arithmetic): a negative low half borrows from the high.
__device__ __forceinline__ uint32_t pk_signed(uint32_t v) { return v - ((v & 0x8000u) << 1); }
template <int M, bool SOP>
__device__ __forceinline__ void cell_messages_vi(
    const uint32_t (&a)[M], const uint32_t (&b)[M], const uint32_t (&c)[M],
    const uint32_t (&SBC)[M], const uint32_t (&K)[M], const uint32_t (&DMC)[M], const uint32_t (&DMB)[M],
    const PencilArgs &pa,
    const uint32_t (&inIx)[M], const uint32_t (&inIy)[M], const uint32_t (&inIz)[M],
    const uint32_t (&inIxy)[M], const uint32_t (&inIyz)[M], const uint32_t (&inIxz)[M],
    const uint32_t (&inM)[M], uint32_t (&nIx)[M], uint32_t (&oIy)[M], uint32_t (&oIz)[M],
    uint32_t (&oIxy)[M], uint32_t (&oIyz)[M], uint32_t (&oIxz)[M], uint32_t (&oBest)[M]) {
  const uint32_t LAM = pa.i_lam, CP = pa.i_cP, DO = pa.i_dO;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const uint32_t eab = a[i] & b[i], eac = a[i] & c[i];
    const uint32_t sXY = pk_mad(eab, DMB[i], inIxy[i]);
    const uint32_t sXZ = pk_mad(eac, DMC[i], inIxz[i]);
    const uint32_t sYZ = inIyz[i] + SBC[i];  // SBC, SOP's K: pk_signed words
    uint32_t sM;
    if constexpr (SOP) sM = pk_mad(eab, DMB[i], pk_mad(eac, DMC[i], inM[i])) + K[i];
    else sM = pk_mad(eab, K[i], inM[i]);
    const uint32_t sX = inIx[i], sY = inIy[i], sZ = inIz[i];
    const uint32_t Gx = imax3(sY, sZ, sYZ), Gy = imax3(sX, sZ, sXZ), Gz = imax3(sX, sY, sXY);
    const uint32_t best = imax3(Gx, Gy, imax(sXY, sM));
    const uint32_t b1 = best - DO;
    const uint32_t pXY = imax(Gz, b1), pYZ = imax(Gx, b1), pXZ = imax(Gy, b1);
    const uint32_t qXY = pXY - CP, qYZ = pYZ - CP, qXZ = pXZ - CP;
    oBest[i] = best;
    oIxy[i] = pXY;
    oIyz[i] = pYZ;
    oIxz[i] = pXZ;
    nIx[i] = imax3(sX - LAM, qXY, qXZ);
    oIy[i] = imax3(sY - LAM, qXY, qYZ);
    oIz[i] = imax3(sZ - LAM, qYZ, qXZ);
  }
}

// ---------------------------------------------------------------------------
// End search of the helix (pencil_kernel END). A position keeps
// one 32-bit key per half,
//   [31:20] score + 2048   [19:8] 4095 - (x - 1)   [7:0] 255 - lap,
// folded with an unsigned max over the real cells it computes: the largest key
// is the best score at the smallest x, then (the wave, hence y mod NW, being
// fixed) the smallest y. z and the wave join the key after the loop
// (end_key64). Any order of folding gives the same key. The host admits only
// shapes whose fields fit (pencil_ends_admit): x - 1 <= 4095, lap <= 255, and
// every score within +-2048 by use_f16.
//
// At one step the positions of a wave fall into two classes, each with
// wave-uniform terms: those that have wrapped (k <= xpos0) compute x - 1 =
// xpos0 - k of row lap0, the others x - 1 = xpos0 + P - k of row lap0 - 1. So
// is the potential lam (x + y + z) of the V-space forms: x + z = xq + 2 for the
// whole class. EndClass holds, for cells x - 1 = xq - k of row `row` (0-based):
//   start, width  real candidates are the positions start <= k < start + width
//                 (x <= la, the row started and <= lb; face mode: x = la or
//                 y = lb); widthz the same for the position z = lc, whose
//                 cells are all on a face
//   add           what turns a half's value into its key but for k << 8
constexpr uint32_t END_XBITS = 12, END_XMASK = (1u << END_XBITS) - 1u, END_LAPBITS = 8, END_LAPMASK = 255u;
struct EndClass {
  uint32_t start, width, widthz, add;
};
// VI: a half is bias + 8 V, so (half - bias - 8 lam q) << 17 puts score at bit 20
template <bool VI>
__device__ __forceinline__ EndClass end_class(const PencilArgs &pa, int32_t xq, int32_t lap, int32_t row,
                                              int32_t la, int32_t lb) {
  const bool ok = lap >= 0 && row < lb;
  const int32_t lim = ok ? la : 0;
  const int32_t q = xq + row + 3;  // x + y + z of the class
  const int32_t top = VI ? (16384 - pa.bias - 8 * pa.lam * q) : (2048 - pa.lam * q);
  // Each term goes to a VGPR by a v_mov of its own. Left to the compiler, the
  // scalar chain behind them (xpos0, lap0) has so many vector users that it
  // is moved to the VALU as a whole, and the step's scalar operands with it.
  auto to_v = [](uint32_t s) -> uint32_t {
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return v;
  };
  EndClass e;
  e.start = to_v((uint32_t)(xq - lim + 1));
  e.widthz = to_v((uint32_t)lim);
  e.width = to_v(pa.end_face ? (uint32_t)(!ok ? 0 : row + 1 == lb ? la : 1) : (uint32_t)lim);
  e.add = to_v(((uint32_t)top << (VI ? 17 : 20)) + ((uint32_t)((int32_t)END_XMASK - xq) << END_LAPBITS) +
               (uint32_t)((int32_t)END_LAPMASK - lap));
  return e;
}
// Fold register `best` (positions k0 and k0 + 64 M in its halves) into their keys.
template <int M, bool VI, bool FACE>
__device__ __forceinline__ void end_fold(uint32_t best, uint32_t k0, uint32_t kz, const EndClass &eA,
                                         const EndClass &eB, uint32_t &key_lo, uint32_t &key_hi) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k = k0 + 64u * M * h;
    uint32_t hv;  // the half's value at the score field (modulo 2^32: the sum below is exact)
    if constexpr (VI) {
      hv = (h ? best >> 16 : best) << 17;
    } else {
      const _Float16 f = __builtin_bit_cast(_Float16, (uint16_t)(h ? best >> 16 : best));
      hv = (uint32_t)(int32_t)(float)f << 20;
    }
    const uint32_t wa = FACE ? (k == kz ? eA.widthz : eA.width) : eA.width;
    const uint32_t wb = FACE ? (k == kz ? eB.widthz : eB.width) : eB.width;
    const bool inA = k - eA.start < wa, inB = k - eB.start < wb;  // unsigned: start <= k < start + width
    const uint32_t cand = hv + (inA ? eA.add : eB.add) + (k << END_LAPBITS);
    uint32_t &key = h ? key_hi : key_lo;
    key = max(key, (inA || inB) ? cand : 0u);
  }
}
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// A position's key with its wave w and position k: {score : ~(x-1)} : ~y : ~z
__device__ __forceinline__ uint64_t end_key64(uint32_t key, uint32_t w, int NW, uint32_t k) {
  const uint32_t y = (END_LAPMASK - (key & END_LAPMASK)) * (uint32_t)NW + w + 1u, z = k + 1u;
  return ((uint64_t)(key >> END_LAPBITS) << 32) | ((0xFFFFu - y) << 16) | (0xFFFFu - z);
}

// End search of the literal helix (literal_kernel END). A half
// holds a full 16-bit word (score_bits up to 16), x - 1 <= 4094 and the lap up
// to 511 (literal_shape_ok), 37 bits in all, so a position keeps two registers
// per half: the key
//   [31:16] half ^ 0x8000   [15:0] 4095 - (x - 1)
// (the shifted int16 half orders as the wrapped word does, the flipped sign bit
// makes that the unsigned order) and the lap of the key's last update. The key
// is replaced on strictly greater only: a position meets its laps in ascending
// order, so among equal {score, x} the first one kept is the smallest y. This
// fold depends on the order of the steps (tools/literal_emu.py replays it). A
// real cell's key is never 0 (x <= 4095), so 0 is "no candidate yet".
//
// Classes as end_class's, with x = x': a position that has wrapped (k < xpos0)
// is at x = xpos0 - k of row lap0 NW + w + 1, the others at x = xpos0 + P - k
// of the row NW above. LitEndClass holds, for cells x = xq - k of row `row`
// (0-based) in lap `lap`:
//   start, width  real candidates are start <= k < start + width (1 <= x <= la,
//                 the row started and <= lb; face mode: x = la or y = lb);
//                 widthz the same for the position z = lc, all on a face
//   add           4095 - (x - 1) but for k;  lap: the lap itself
struct LitEndClass {
  uint32_t start, width, widthz, add, lap;
};
__device__ __forceinline__ LitEndClass lit_end_class(int32_t face, int32_t xq, int32_t lap, int32_t row,
                                                     int32_t la, int32_t lb) {
  const bool ok = lap >= 0 && row < lb;
  const int32_t lim = ok ? la : 0;
  auto to_v = [](uint32_t s) -> uint32_t {  // (end_class: one v_mov per term keeps the chain scalar)
    uint32_t v;
    asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return v;
  };
  LitEndClass e;
  e.start = to_v((uint32_t)(xq - lim));
  e.widthz = to_v((uint32_t)lim);
  e.width = to_v(face ? (uint32_t)(!ok ? 0 : row + 1 == lb ? la : 1) : (uint32_t)lim);
  e.add = to_v((uint32_t)(4096 - xq));
  e.lap = to_v((uint32_t)lap);
  return e;
}
// Fold register `best` (the MAX7 of positions k0 and k0 + 64 M, in its halves)
// into their keys and laps.
template <int M, bool FACE>
__device__ __forceinline__ void lit_end_fold(uint32_t best, uint32_t k0, uint32_t kz, const LitEndClass &eA,
                                             const LitEndClass &eB, uint32_t (&key)[2], uint32_t (&klap)[2]) {
  const uint32_t bx = best ^ 0x80008000u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k = k0 + 64u * M * h;
    const uint32_t hv = h ? (bx & 0xFFFF0000u) : (bx << 16);
    const uint32_t wa = FACE ? (k == kz ? eA.widthz : eA.width) : eA.width;
    const uint32_t wb = FACE ? (k == kz ? eB.widthz : eB.width) : eB.width;
    const bool inA = k - eA.start < wa, inB = k - eB.start < wb;  // unsigned: start <= k < start + width
    const uint32_t cand = (inA || inB) ? hv + (inA ? eA.add : eB.add) + k : 0u;
    const bool up = cand > key[h];
    key[h] = up ? cand : key[h];
    klap[h] = up ? (inA ? eA.lap : eB.lap) : klap[h];
  }
}
// A position's key with its lap, wave w and position k: {score : ~(x-1)} : ~y : ~z
__device__ __forceinline__ uint64_t lit_end_key64(uint32_t key, uint32_t lap, uint32_t w, int NW, uint32_t k) {
  const uint32_t y = lap * (uint32_t)NW + w + 1u, z = k + 1u;
  return ((uint64_t)key << 32) | ((0xFFFFu - y) << 16) | (0xFFFFu - z);
}

// Shift a packed per-position value one position up the helix (k <- k-1).
// With k = 64M*h + M*lane + i, register i >= 1 takes register i-1 of the same
// lane (a rename, no instruction); register 0 takes register M-1 of lane-1
// (one DPP wave_ror:1), except lane 0: its low half is position 0 and gets the
// z = 0 face, its high half (position 64M) takes the low half of lane 63's
// register M-1 -- one v_perm with a per-lane selector does both.
// Only lane 0 reads the second v_perm source (its selector takes bytes 2..3 of
// it), so that source is `face`, whose high half is the z = 0 face (or, for a
// z-tile, the previous tile's last position) -- no extra v_bfi.
template <int M>
__device__ __forceinline__ void zshift(uint32_t (&v)[M], const uint32_t (&src)[M], uint32_t sel,
                                       uint32_t face) {
  const uint32_t r = ror1(src[M - 1]);
#pragma unroll
  for (int i = M - 1; i >= 1; --i) v[i] = src[i - 1];
  v[0] = __builtin_amdgcn_perm(r, face, sel);
}
// The same for values read at position k-1 already (the reader aimed its LDS
// read at the previous position's record): only lane 0's register 0 changes,
// {face, lane 63's low half}; the v_perm passes every other lane's through.
template <int M>
__device__ __forceinline__ void zfix(uint32_t (&v)[M], const uint32_t (&src)[M], uint32_t sel, uint32_t face) {
#pragma unroll
  for (int i = M - 1; i >= 1; --i) v[i] = src[i];
  v[0] = __builtin_amdgcn_perm(src[0], face, sel);
}
// A codes of a lane's M registers: entries va, va-4, ... of the LDS table
// (register i holds position M*lane+i, one x behind register i-1).
template <int M>
__device__ __forceinline__ void load_a(uint32_t va, uint32_t (&a)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i)
    a[i] = *(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)(
        va + 4u * (uint32_t)(M - 1 - i));
}
// The same at a constant entry offset `off` from va, as an inbounds index of
// an LDS pointer, so the offset folds into the ds_read's offset field (a u32
// add could wrap, and the compiler then adds it in a VALU op)
template <int M>
__device__ __forceinline__ void load_a_off(uint32_t va, int off, uint32_t (&a)[M]) {
  const __attribute__((address_space(3))) uint32_t *p =
      (const __attribute__((address_space(3))) uint32_t *)(uintptr_t)va;
#pragma unroll
  for (int i = 0; i < M; ++i) a[i] = p[off + M - 1 - i];
}
// V-space, M = 2: entries OFF and OFF + 1 of va's table as one ds_read_b64
// (a[1] = entry OFF, a[0] = OFF + 1). The group's first entry va is odd, so
// the pair is 8-byte aligned in the table itself for odd OFF, and in the copy
// shifted by one entry (va_s: entry j holds the table's j + 1) for even OFF.
// Lanes 8 B apart then read 512 contiguous bytes, conflict-free in both
// 32-lane groups; ds_read2_b32 is serviced as two ds_read_b32 banked mod 32,
// which lanes two dwords apart make 2-way (MI355X_MICROARCH.md, LDS).
template <int OFF>
__device__ __forceinline__ void load_a_pair(uint32_t va, uint32_t va_s, uint32_t (&a)[2]) {
  const uint32_t addr = (OFF & 1) ? va + 4u * OFF : va_s + 4u * (OFF - 1);
  // one 64-bit integer load (a uint2 is split into two dword loads, which the
  // backend re-merges into ds_read2_b32 unless it can prove the alignment)
  const uint64_t v = *(const __attribute__((address_space(3))) uint64_t *)(uintptr_t)addr;
  a[1] = (uint32_t)v;
  a[0] = (uint32_t)(v >> 32);
}
// Position k -> (lane, register, half) of the layout above.
template <int M>
__device__ __forceinline__ void pos_split(int32_t k, int32_t &l, int32_t &i, int32_t &h) {
  const uint32_t u = (uint32_t)k;  // k >= 0: shifts and masks only (M is a power of 2)
  h = (int32_t)(u / (64u * M));
  l = (int32_t)((u / M) & 63u);
  i = (int32_t)(u % M);
}

// The step lambdas are left to the regular inliner for M <= 2 (an early forced
// inline costs ~7 % there); for M >= 4 the inliner gives up on their size and
// the captured state would spill to scratch, so those calls are forced inline.
// So are the end search's (END): the fold makes the step too large as well.
#define TSA_INLINE_IF_WIDE(call)                 \
  do {                                           \
    if constexpr (M >= 4 || END) {               \
      [[clang::always_inline]] call;             \
    } else {                                     \
      call;                                      \
    }                                            \
  } while (0)

// Host: packed constants of a parameter set (pencil_kernel.hip).
// vi_bias: the integer-pattern V-space cell's bias (0: the float cell)
PencilArgs make_args(const KParams &kp, bool f16, bool vs, int32_t vi_bias = 0);

// Instantiated helix shapes: M = 1, 2, 4, 8 pairs per lane (LC up to 128 M),
// 8 rows per workgroup; each in f16 / int16 arithmetic and RTL / SOP s3.
#define TSA_SHAPES(LAUNCH, M_, F16_, SOP_, ...)                                            \
  ((M_) == 1 ? TSA_ARITH(LAUNCH, 1, 8, F16_, SOP_, __VA_ARGS__)                            \
   : (M_) == 2 ? TSA_ARITH(LAUNCH, 2, 8, F16_, SOP_, __VA_ARGS__)                          \
   : (M_) == 4 ? TSA_ARITH(LAUNCH, 4, 8, F16_, SOP_, __VA_ARGS__)                          \
               : TSA_ARITH(LAUNCH, 8, 8, F16_, SOP_, __VA_ARGS__))
#define TSA_ARITH(LAUNCH, MM, NN, F16_, SOP_, ...)                                        \
  ((F16_) ? ((SOP_) ? LAUNCH<MM, NN, true, true>(__VA_ARGS__)                              \
                    : LAUNCH<MM, NN, true, false>(__VA_ARGS__))                            \
          : ((SOP_) ? LAUNCH<MM, NN, false, true>(__VA_ARGS__)                             \
                    : LAUNCH<MM, NN, false, false>(__VA_ARGS__)))

}  // namespace tsa
