// h_table.h -- f16 bits of the small non-negative integers, built at compile
// time (plain C++17: the helix kernel reads it through scalar loads, and a host
// test compiles this header alone).
//
// Entry v holds the IEEE f16 bits of the integer v in both 16-bit halves,
// exact for v <= 2047; every entry from 2047 on repeats the 2047 entry. The
// V-space helix's face values H = lam q are such integers: below 2048 at every
// real cell (use_vs), larger only at padding positions, whose reader clamps
// its index into the saturated tail (pencil_kernel.hip, TSA_H_TAB).
#pragma once

#include <cstdint>

namespace tsa {

constexpr int H_TAB_SAT = 2047;  // the largest integer encoded
// a clamped four-entry read starts at H_TAB_SAT + 1 at the most
constexpr int H_TAB_N = H_TAB_SAT + 1 + 4;

constexpr uint32_t f16x2_of_int(uint32_t v) {
  if (v == 0) return 0u;
  if (v > (uint32_t)H_TAB_SAT) v = H_TAB_SAT;
  int e = 0;
  while ((v >> (e + 1)) != 0) ++e;                           // 2^e <= v < 2^(e+1), e <= 10
  const uint32_t bits = ((uint32_t)(e + 15) << 10) | ((v << (10 - e)) & 0x3FFu);
  return bits * 0x00010001u;
}

struct HTable {
  uint32_t v[H_TAB_N];
};
constexpr HTable make_h_table() {
  HTable t{};
  for (int i = 0; i < H_TAB_N; ++i) t.v[i] = f16x2_of_int((uint32_t)i);
  return t;
}

}  // namespace tsa
