// lap_kernel_body.h -- the body of lap_kernel and lap_ends_kernel
// (lap_kernel.hip), included inside each of the two __global__ functions: it
// reads their parameters (seqs_ .. lit_, ekey_) and the constants M, NW, F16,
// SOP, CHK, SYS, LIT, VS and END, template parameters of lap_kernel and
// constants of lap_ends_kernel. Not a header of its own.
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  static_assert(!END || (CHK && !F16 && !SYS && !LIT && !VS), "the end search: the checked int16 form");
  static_assert(!(CHK && F16), "the checked kernel runs the int16 form");
  static_assert(!(CHK && SYS), "a split cube runs the unchecked forms");
  static_assert(!(LIT && (F16 || CHK)), "the literal form: int16, unchecked");
  static_assert(!VS || (F16 && !CHK && !LIT && !SYS), "V-space: the f16 single-device form");
  // the loader writes the step-varying y = 0 / z = 0 faces (LIT, VS)
  constexpr bool FACES = LIT || VS;
  // four-step groups (TSA_LAP_U4) for M <= 2 (M = 4's checked form spills with
  // them), their VGPR bases (TSA_LAP_VBASE) but for the M = 1 factored int16
  // forms (at the 80-VGPR cap of two NW = 8 workgroups per CU they spill 8 bytes)
  constexpr bool U4K = TSA_LAP_U4 && M <= 2;
  constexpr bool VBK = TSA_LAP_VBASE && U4K && (F16 || LIT || M == 2);
  // the loader's record loads and progress-word period (TSA_LAP_L16 / _PROGP)
  constexpr bool FM1 = M == 1;
  constexpr int L16K = TSA_LAP_L16 >= 0 ? TSA_LAP_L16 : FM1 ? 2 : 0;
  constexpr int PROGPK = TSA_LAP_PROGP >= 0 ? TSA_LAP_PROGP : FM1 ? 4 : 2;
  constexpr int SCOPE = SYS ? __HIP_MEMORY_SCOPE_SYSTEM : __HIP_MEMORY_SCOPE_AGENT;
  constexpr int RW = 2 * NW, ZT = 64 * M, LPD = lap_pd(M), K = lap_k(M), K0 = lap_k0(M);
  constexpr int PAIR = 64 * REC_BYTES, SLOT = M * PAIR;
  // wave w's rows sit at step offsets 2w (low half) and 2w + 1 (high); lap L+1
  // reads lap L's record t + YOFF; loader step s checks y record s + YOFF and
  // z record s + ZT + ZA (ZA = NW: every wave's z reads stay covered)
  constexpr int YOFF = 2 * (NW - 1) + 1, ZA = NW;
  constexpr int ZREC = NW * LAP_ZREC_WAVE, OFF = ZT + 2 * NW;
  uint8_t *xr = smem;
  uint8_t *xr0 = xr + (NW - 1) * K * SLOT;
  uint8_t *zring = xr0 + K0 * SLOT;
  uint8_t *yface = zring + LAP_ZL * ZREC;
  uint8_t *zface = yface + SLOT;
  int32_t *wd = (int32_t *)(zface + ZREC);
  int32_t *pw = wd + 16;
  uint32_t *fin = (uint32_t *)(pw + 64 * (NW + 1));
  uint32_t *sA2 = fin + lap_fin_words(M, LIT);
  int32_t *const w_bp = wd + 9, *const w_abort = wd + 12, *const bpw = wd + 13, *const w_stall = wd + 15;

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // w == NW: the loader
  // block -> (lap, column): column c = tri*GZ + q (one z-tile of one triple), block
  // b = 8 * (L*CH + c/8) + c%8 -- a column's laps share b % 8 (one XCD), and
  // every producer ((L-1, c), (L, c-1)) has a lower block index than its consumer
  // Dispatch rounds are a loop, not a hope: the grid holds one round (every
  // workgroup resident), and physical block p runs the logical blocks of
  // slots p/8, p/8 + SX, p/8 + 2 SX, ... of its XCD one after another -- lap
  // order per physical workgroup whatever the dispatcher does, and a slot's
  // next lap starts the moment its previous one ends. One round: one pass.
  auto lap_body = [&](const int32_t slot) {
  const uint8_t *__restrict__ seqs = seqs_;
  const int64_t *__restrict__ offs = offs_;
  const int32_t G = G_, GZ = GZ_, NC = NC_, CH = CH_, YR = YR_, ZR = ZR_;
  uint8_t *__restrict__ yf_base = yf_base_, *__restrict__ zf_base = zf_base_;
  const LapRounds &rd = rd_;
  int32_t *__restrict__ prog = prog_;
  uint32_t *__restrict__ err = err_;
  int32_t *__restrict__ scores = scores_, *__restrict__ mon = mon_;
  const PencilArgs &pa = pa_;
  const uint32_t epoch = epoch_, spin_limit = spin_limit_;
  const int32_t L0 = L0_, L1 = L1_;
  uint8_t *__restrict__ yf_out = yf_out_;
  int32_t *__restrict__ prog_in = prog_in_;
  unsigned long long *__restrict__ trace = trace_;
  const LitArgs &lit = lit_;
  const int32_t b = 8 * slot + (int32_t)(blockIdx.x & 7);  // logical block
  // the lane / thread index laundered per lap: otherwise the compiler hoists
  // every per-lane address out of the round loop and keeps it live across
  // the whole body (+20 VGPRs, measured), where one pass rematerialises them
  int32_t tid = (int32_t)threadIdx.x;
#if TSA_LAP_LAUNDER
  asm volatile("" : "+v"(tid));
#endif
  const int lane = tid & 63;
  const int32_t L = L0 + slot / CH, col = (slot % CH) * 8 + (b & 7);
  if (col >= NC || L >= L1) return;  // padding block
  const int32_t tri = col / GZ, q = col % GZ;
  const int64_t o0 = offs[3 * (int64_t)tri], o1 = offs[3 * (int64_t)tri + 1];
  const int64_t o2 = offs[3 * (int64_t)tri + 2], o3 = offs[3 * (int64_t)tri + 3];
  const int32_t la = (int32_t)(o1 - o0), lb = (int32_t)(o2 - o1), lc = (int32_t)(o3 - o2);
  const int32_t nlap = (lb + RW - 1) / RW, ntile = (lc + ZT - 1) / ZT;
  if (L >= nlap || q >= ntile) return;  // beyond this triple's own laps / tiles
  auto stamp = [&](int s, unsigned long long v) {
    if (trace != nullptr && tid == 0) trace[(int64_t)b * LAP_TRACE_SLOTS + s] = v;
  };
  auto now = [&]() {
    unsigned long long v;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
    return v;
  };
  if (trace != nullptr) {
    stamp(0, now());
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    stamp(3, x);
  }
  const int64_t lid = ((int64_t)tri * G + L) * GZ + q;  // logical workgroup id
  const bool yin = L > 0, zin = q > 0, yout = L + 1 < nlap, zout = q + 1 < ntile;
  const int32_t zt_q = min(ZT, lc - q * ZT), rows = min(RW, lb - L * RW);
  const bool final_wg = !yout && !zout;
  auto tau = [](int32_t r) { return 2 * (r >> 1) + (r & 1); };  // step offset of lap row r
  const int32_t r_f = lb - 1 - L * RW, k_f = lc - 1 - q * ZT;
  constexpr int32_t LX = LIT ? 1 : 0;  // LIT: x' = 0 .. la, one step more
  const int32_t T = final_wg ? (la - 1 + LX) + tau(r_f) + k_f + 1 : la + LX + tau(rows - 1) + zt_q - 1;
  const int32_t T_above = la + LX + tau(RW - 1) + zt_q - 1;  // records the lap above writes (same tile)
  const int32_t T_left = la + LX + tau(rows - 1) + ZT - 1;   // z records the tile to the left writes
  // Rings. A grid beyond the resident slots runs in rounds of rd.SX slots per
  // XCD, each resident workgroup looping over its slots in lap order (the
  // slot loop at the end of lap_kernel). A producer whose consumer is in a later
  // round gets a full-length ring from the boundary region (it never waits
  // for a consumer that may not have started); all others a slim ring of
  // YR / ZR slots, their consumers co-resident (lap_geom).
  const int32_t ch = slot % CH, xc = b & 7;
  auto round_of = [&](int32_t s) { return s / rd.SX; };
  auto y_bidx = [&](int32_t Lp, int32_t sp) {  // boundary index of producer (Lp, my column), or -1
    const int32_t sc = sp + CH;
    if (round_of(sc) == round_of(sp)) return -1;
    return (int32_t)(((int64_t)col * rd.KBY) + (CH >= rd.SX ? Lp - L0 : round_of(sp) - round_of(ch)));
  };
  auto z_bidx = [&](int32_t sp, int32_t xp) {  // boundary index of producer (slot sp, XCD xp), or -1
    return (xp == 7 && round_of(sp + 1) != round_of(sp)) ? round_of(sp) : -1;
  };
  const int32_t yb_me = yout ? y_bidx(L, slot) : -1, yb_pr = yin ? y_bidx(L - 1, slot - CH) : -1;
  const int32_t zb_me = zout ? z_bidx(slot, xc) : -1;
  const int32_t zb_pr = zin ? (xc == 0 ? z_bidx(slot - 1, 7) : -1) : -1;
  const int32_t YRm = yb_me >= 0 ? rd.YRB : YR, YRp = yb_pr >= 0 ? rd.YRB : YR;
  const int32_t ZRm = zb_me >= 0 ? rd.ZRB : ZR, ZRp = zb_pr >= 0 ? rd.ZRB : ZR;
  uint8_t *yf_mine = yb_me >= 0 ? rd.yb + (int64_t)yb_me * rd.YRB * SLOT
                                : (L == L1 - 1 ? yf_out : yf_base) + lid * YR * SLOT;  // in my consumer's memory
  // my progress word: read by the z producer (same part, local) and the y
  // producer -- at lap L0 of a split cube the previous part, so a copy goes there
  int32_t *const prog_x = (SYS && L == L0 && L0 > 0) ? prog_in + lid * LAP_PROG_STRIDE : nullptr;
  const uint8_t *yf_prev = !yin ? yf_mine
                           : yb_pr >= 0 ? rd.yb + (int64_t)yb_pr * rd.YRB * SLOT
                                        : yf_base + (lid - GZ) * YR * SLOT;
  uint8_t *zf_mine = zb_me >= 0 ? rd.zb + (int64_t)zb_me * rd.ZRB * ZREC : zf_base + lid * ZR * ZREC;
  const uint8_t *zf_prev = !zin ? zf_mine
                           : zb_pr >= 0 ? rd.zb + (int64_t)zb_pr * rd.ZRB * ZREC
                                        : zf_base + (lid - 1) * ZR * ZREC;
  const uint32_t ep19 = epoch & 0x7FFFFu;
  bool timed_out = false;
  auto fail = [&]() {  // every wait of this workgroup gives up from now on
    if (!timed_out && lane == 0) {
      __hip_atomic_store(err, epoch, __ATOMIC_RELEASE, SCOPE);
      *(volatile __attribute__((address_space(3))) int32_t *)(__attribute__((address_space(3))) void *)w_abort = 1;
    }
    timed_out = true;
  };
  // wait until an LDS progress word reaches `need` (bounded: a hand-off timeout
  // upstream aborts the workgroup, and no wait outlives ~4 x spin_limit polls)
  uint32_t n_wait = 0;
  auto wait_word = [&](const int32_t *word, int32_t &seen, int32_t need) {
    if (need <= seen) return;
    seen = lds_word(word);
    if (need <= seen) return;
    ++n_wait;
    for (uint32_t spin = 1;; ++spin) {
      seen = lds_word(word);
      if (need <= seen) return;
      if ((spin & 255) == 0 && (timed_out || lds_word(w_abort) != 0 || spin >= 4 * spin_limit)) {
        fail();
        seen = 1 << 24;
        return;
      }
      if (spin > 64) __builtin_amdgcn_s_sleep(1);
    }
  };

  // ---- A code pairs, zeroed words
  const int32_t na = lap_na(la, M, NW, LIT);
  for (int j = tid; j < na; j += 64 * (NW + 1)) {
    const int x0 = j - OFF, x1 = j - OFF - 1;
    const uint32_t c0 = (x0 >= 0 && x0 < la) ? SYM0 << tsa_sym(seqs, o0 + x0, pa.packed) : 0u;
    const uint32_t c1 = (x1 >= 0 && x1 < la) ? SYM0 << tsa_sym(seqs, o0 + x1, pa.packed) : 0u;
    sA2[j] = c0 | (c1 << 16);
  }
  if (tid < 16) wd[tid] = 0;
  // face records, so a lap-0 wave 0 / tile-0 wave reads its y / z inputs the
  // same way as any other (no branch in the step): y {Iy, Ixy | Iyz, best} low
  // halves (wave 0's perm format), z {Iz, -, Ixz, - | Iyz, -, M, -}
  for (int j = tid; j < M * 64; j += 64 * (NW + 1))
    ((uint4 *)yface)[j] = make_uint4((pa.f_single & 0xFFFFu) | (pa.f_pair & 0xFFFF0000u), 0u,
                                     pa.f_pair & 0xFFFFu, 0u);
  if (tid < 2 * NW)
    ((uint4 *)zface)[tid] = (tid & 1) ? make_uint4(pa.f_pair, 0u, 0u, 0u)
                                                      : make_uint4(pa.f_single, 0u, pa.f_pair, 0u);
  if constexpr (U4K && !FACES) {  // the same records in every ring slot (no loader writes)
    if (!yin)
      for (int j = tid; j < K0 * M * 64; j += 64 * (NW + 1))
        ((uint4 *)xr0)[j] = make_uint4((pa.f_single & 0xFFFFu) | (pa.f_pair & 0xFFFF0000u), 0u,
                                       pa.f_pair & 0xFFFFu, 0u);
    if (!zin)
      for (int j = tid; j < LAP_ZL * 2 * NW; j += 64 * (NW + 1))
        ((uint4 *)zring)[j] = (j & 1) ? make_uint4(pa.f_pair, 0u, 0u, 0u)
                                      : make_uint4(pa.f_single, 0u, pa.f_pair, 0u);
  }
  pw[tid] = 0;  // blockDim = 64 (NW + 1): one word per thread
  // the wave-to-wave rings: step 0 reads slot K-1 before any write (its cells
  // are not real, but the checked kernel's monitor must not see stale LDS)
  for (int j = tid; j < (NW - 1) * K * SLOT / 16; j += 64 * (NW + 1))
    ((uint4 *)xr)[j] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  if (w == NW) {
    // =================== loader wave ===================
    // Records are fetched LPD steps ahead into registers with 8-byte sc1 loads
    // (one {payload, tag} granule each: relaxed agent-scope atomics, so the
    // compiler counts vmcnt itself), their tags checked in registers, then
    // written to LDS (xr0 / zring) and published.
    uint32_t stalls = 0;
    typedef unsigned long long u64;
    // TSA_LAP_L16: a record's two granules by one 16-byte load (volatile:
    // sc0 sc1, L1 bypassed, L2-served; each naturally aligned 8-byte {payload,
    // tag} granule of it is untorn, so the per-granule tag check stands)
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    auto gl16 = [&](const uint8_t *p) -> u64x2 {
      return *(volatile const __attribute__((address_space(1))) u64x2 *)(
          const __attribute__((address_space(1))) void *)p;
    };
    // TSA_LAP_L16 = 2: the same 16 bytes by a raw buffer load with sc1 (a
    // compiler-counted load, no vmcnt(0) behind it), off a per-lap resource
    // of the ring's base
    // (TSA_LAP_NOFACE_FETCH: a lap-0 / tile-0 loader, whose y / z fetches feed
    // nothing, gets a zero-length resource -- its loads stay in the window, so
    // the compiler's vmcnt counting stays static, but return 0 without a
    // memory access)
    const int32_t ny = (TSA_LAP_NOFACE_FETCH && !yin) ? 0 : 0x7FFFFFFF;
    const int32_t nz = (TSA_LAP_NOFACE_FETCH && !zin) ? 0 : 0x7FFFFFFF;
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void *)yf_prev, (short)0, ny, 0x00020000);
    const __amdgpu_buffer_rsrc_t rzr = __builtin_amdgcn_make_buffer_rsrc((void *)zf_prev, (short)0, nz, 0x00020000);
    auto bl16 = [&](__amdgpu_buffer_rsrc_t r, uint32_t off) -> u64x2 {
      if constexpr (SYS)  // 17: sc0 sc1 (system scope, as the 8-byte loads of the split)
        return __builtin_bit_cast(u64x2, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 17));
      else  // 16: sc1
        return __builtin_bit_cast(u64x2, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16));
    };
    auto gl8 = [&](const uint8_t *p) -> u64 {
      return __hip_atomic_load((const u64 *)p, __ATOMIC_RELAXED, SCOPE);
    };
    const int64_t cons_y = yout ? lid + GZ : lid, cons_z = zout ? lid + 1 : lid;
    struct Fetch {
      u64 y[2 * M], z[2];
      int32_t py, pz;  // my consumers' progress words (lane 0)
    };
    auto fetch_y = [&](int32_t s, Fetch &f) {  // y record s + YOFF
      const int32_t r = s + YOFF;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const uint8_t *g = yf_prev + ((int64_t)(r & (YRp - 1)) * M + i) * PAIR + lane * REC_BYTES;
        if constexpr (L16K == 2) {
          const u64x2 v = bl16(ry, (uint32_t)(((int64_t)(r & (YRp - 1)) * M + i) * PAIR + lane * REC_BYTES));
          f.y[2 * i] = v[0];
          f.y[2 * i + 1] = v[1];
        } else if constexpr (L16K == 1) {
          const u64x2 v = gl16(g);
          f.y[2 * i] = v[0];
          f.y[2 * i + 1] = v[1];
        } else {
          f.y[2 * i] = gl8(g);
          f.y[2 * i + 1] = gl8(g + 8);
        }
      }
    };
    auto fetch_z = [&](int32_t rz, Fetch &f) {  // z record rz (lanes 0 .. 2NW-1)
      const uint8_t *g = zf_prev + (int64_t)(rz & (ZRp - 1)) * ZREC + (lane & (2 * NW - 1)) * 16;
      if constexpr (L16K == 2) {
        const u64x2 v = bl16(rzr, (uint32_t)((int64_t)(rz & (ZRp - 1)) * ZREC + (lane & (2 * NW - 1)) * 16));
        f.z[0] = v[0];
        f.z[1] = v[1];
      } else if constexpr (L16K == 1) {
        const u64x2 v = gl16(g);
        f.z[0] = v[0];
        f.z[1] = v[1];
      } else {
        f.z[0] = gl8(g);
        f.z[1] = gl8(g + 8);
      }
    };
    auto fetch = [&](int32_t s, Fetch &f, bool progw = true) {
      fetch_y(s, f);
      fetch_z(s + ZT + ZA, f);
      if (progw) {
        f.py = __hip_atomic_load(prog + cons_y * LAP_PROG_STRIDE, __ATOMIC_RELAXED, SCOPE);
        f.pz = __hip_atomic_load(prog + cons_z * LAP_PROG_STRIDE, __ATOMIC_RELAXED, SCOPE);
      }
    };
    // LIT: the y = 0 (lap 0) and z = 0 (tile 0) faces, written into the rings
    // wave 0 and position 0 read: zero cells pushing with the receivers'
    // symbols (tools/litlap_emu.py zero_push), so they vary with the step
    uint32_t lones = 0x00010001u, lb1 = 0, lc1 = 0, lby2 = 0, lcn[M], lfyz[M];
    LitArgs cv = lit;
    if constexpr (LIT) {
      asm volatile("" : "+v"(lones), "+v"(cv.dmS), "+v"(cv.d1S), "+v"(cv.d0S), "+v"(cv.neS), "+v"(cv.mm3S),
                   "+v"(cv.fP[0]), "+v"(cv.fP[1]));
      auto code = [&](int64_t base, int32_t i, int32_t len) -> uint32_t {
        return (i >= 0 && i < len) ? SYM0 << tsa_sym(seqs, base + i, pa.packed) : 0u;
      };
      lb1 = code(o1, 0, lb) * 0x00010001u;  // b_1 (the y = 0 face is lap 0's)
      lc1 = code(o2, 0, lc) * 0x00010001u;  // c_1
      const int32_t yz = L * RW + 2 * ((lane & (2 * NW - 1)) >> 1);
      lby2 = code(o1, yz, lb) | (code(o1, yz + 1, lb) << 16);  // b_y of the two rows of wave lane / 2
#pragma unroll
      for (int i = 0; i < M; ++i) {
        lcn[i] = code(o2, q * ZT + M * lane + i + 1, lc) * 0x00010001u;  // c_{z+1}
        lfyz[i] = lit_face_pair(cv, lb1, lcn[i], lones);
      }
    }
    // wave 0's record of step s: row 0's pushes into row 1 at x' = s - k, in
    // the tagged record format (low halves: Iy | Ixy << 16, Iyz | M << 16)
    auto yface_lit = [&](int32_t s, int i) -> uint4 {
      const uint32_t an = sA2[s - (M * lane + i) + OFF] & 0xFFFFu;  // a_{x'+1}
      const uint32_t fxy = lit_face_pair(cv, an, lb1, lones), fm = lit_face_m<SOP>(cv, an, lb1, lcn[i], lones);
      return make_uint4((cv.fS[1] & 0xFFFFu) | (fxy << 16), 0u, (lfyz[i] & 0xFFFFu) | (fm << 16), 0u);
    };
    // z record rz (lanes 0 .. 2NW-1: wave lane / 2, word pair lane & 1): the
    // z = 0 cells of that wave's two rows at x' = rz - ZT + 1 - 2w - h
    auto zface_lit = [&](int32_t rz) -> uint4 {
      const int32_t wz = (lane & (2 * NW - 1)) >> 1;
      const uint32_t a2 = sA2[rz - ZT + 1 - 2 * wz + OFF];  // a_{x'+1}: row 2wz (lo), 2wz + 1 (hi)
      if (lane & 1)
        return make_uint4(lit_face_pair(cv, lby2, lc1, lones), 0u, lit_face_m<SOP>(cv, a2, lby2, lc1, lones), 0u);
      return make_uint4(cv.fS[2], 0u, lit_face_pair(cv, a2, lc1, lones), 0u);
    };
    // VS: the same faces as V-space values -- a face cell at coordinate sum
    // q_f sends lam q_f to a pair target and to M, lam q_f - lam to a single
    // target. Lap 0's record of step s (wave 0's low halves, rows 0 -> 1):
    // Iy = lam (s + zoff + 1), Ixy = Iyz = best = lam (s + zoff + 2), the same
    // on every lane (x + z is the step); tile 0's z record for step t = rz - ZT
    // (position 0 of every wave): Iz = Iyz = M = lam (t + L RW + 2), Ixz one lam more
    const int32_t zoff = q * ZT;
    auto yface_vs = [&](int32_t s) -> uint4 {
      const uint32_t f1 = lam_bits(pa.lam, s + zoff + 1) & 0xFFFFu, f2 = lam_bits(pa.lam, s + zoff + 2) & 0xFFFFu;
      return make_uint4(f1 | (f2 << 16), 0u, f2 | (f2 << 16), 0u);
    };
    auto zface_vs = [&](int32_t rz) -> uint4 {
      const int32_t t = rz - ZT;
      const uint32_t g1 = lam_bits(pa.lam, t + L * RW + 2);
      if (lane & 1) return make_uint4(g1, 0u, g1, 0u);                  // {Iyz, -, M, -}
      return make_uint4(g1, 0u, lam_bits(pa.lam, t + L * RW + 3), 0u);  // {Iz, -, Ixz, -}
    };
    auto tag_ok = [](u64 g, uint32_t tg) { return (uint32_t)(g >> 32) == tg; };
    auto y_ok = [&](int32_t s, const Fetch &f) {
      const uint32_t tg = lap_tag(epoch, s + YOFF);
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 2 * M; ++i) ok = ok && tag_ok(f.y[i], tg);
      return __all(ok) != 0;
    };
    auto z_ok = [&](int32_t rz, const Fetch &f) {
      const uint32_t tg = lap_tag(epoch, rz);
      return __all(lane >= 2 * NW || (tag_ok(f.z[0], tg) && tag_ok(f.z[1], tg))) != 0;
    };
    // slow path: fetch again until the tags match (the producer has not stored yet)
    auto settle_y = [&](int32_t s, Fetch &f) {
      ++stalls;
      for (uint32_t spin = 0;; ++spin) {
        if (spin >= spin_limit || timed_out || ((spin & 63) == 63 && lds_word(w_abort) != 0)) {
          fail();
          return;
        }
        fetch_y(s, f);
        if (y_ok(s, f)) return;
        __builtin_amdgcn_s_sleep(1);
      }
    };
    auto settle_z = [&](int32_t rz, Fetch &f) {
      ++stalls;
      for (uint32_t spin = 0;; ++spin) {
        if (spin >= spin_limit || timed_out || ((spin & 63) == 63 && lds_word(w_abort) != 0)) {
          fail();
          return;
        }
        fetch_z(rz, f);
        if (z_ok(rz, f)) return;
        __builtin_amdgcn_s_sleep(1);
      }
    };
    // records beyond the producer's last step are never checked; they only
    // feed cells past the cube, stored as zeros (the checked kernel's monitor
    // sees those cells too, and must not see stale ring contents)
    auto put_z = [&](int32_t rz, const Fetch &f) {
      const bool real = rz < T_left;
      if (U4K && !FACES && !zin) return;  // zring holds the prefilled z = 0 face
      if (lane < 2 * NW) {
        uint4 v = real ? make_uint4((uint32_t)f.z[0], (uint32_t)(f.z[0] >> 32), (uint32_t)f.z[1],
                                    (uint32_t)(f.z[1] >> 32))
                       : make_uint4(0u, 0u, 0u, 0u);
        if constexpr (LIT) {
          if (!zin) v = zface_lit(rz);
        }
        if constexpr (VS) {
          if (!zin) v = zface_vs(rz);
        }
        lds_write16(zring + (rz & (LAP_ZL - 1)) * ZREC + lane * 16, v);
      }
    };
    int32_t seen_w0 = 0, seen_wl = 0;
    // prologue: z records ZT-2 .. ZT+ZA-1 (position 0's step-0 inputs and the
    // z reads of steps the loader's progress does not cover), checked now
    if (zin || FACES) {  // (LIT / VS tile 0: the z = 0 faces of those records)
      for (int rz = ZT - 2; rz < ZT + ZA; ++rz) {
        Fetch f;
        f.z[0] = f.z[1] = 0;
        if (zin) {
          fetch_z(rz, f);
          if (rz < T_left && !z_ok(rz, f)) settle_z(rz, f);
        }
        put_z(rz, f);
      }
    }
    __syncthreads();  // (matches the compute waves' prologue barrier)
    Fetch fq[LPD];
    // the loop period LU (a multiple of LPD; the effective progress-word refresh
    // period, see TSA_LAP_PROGP): the progress words ride with the fetch
    // processed at phase 0 of a period, issued LPD steps earlier
    constexpr bool PTHIN = PROGPK > 1;
    constexpr int LU = (PROGPK > LPD && PROGPK % LPD == 0) ? PROGPK : LPD;
#pragma unroll
    for (int j = 0; j < LPD; ++j) fetch(j, fq[j], !PTHIN || j == 0);
    // one step: check the fetch of step s (registers fq[j]), store it to LDS,
    // publish, refill fq[j] with step s + LPD
    auto lstep = [&](auto ph, int32_t s) {
      constexpr int PHL = decltype(ph)::value;  // phase in the loop period
      constexpr int j = PHL % LPD;
      Fetch &f = fq[j];
      if (yin && s + YOFF < T_above && !y_ok(s, f)) settle_y(s, f);
      const int32_t rz = s + ZT + ZA;
      if (zin && rz < T_left && !z_ok(rz, f)) settle_z(rz, f);
      constexpr bool PROGW = !PTHIN || PHL == 0;  // this fetch carries the progress words
      if (PROGW && lane == 0) {  // my consumers' progress, for the producing waves' back-pressure
        bpw[0] = f.py;
        bpw[1] = f.pz;
      }
      wait_word(pw, seen_w0, s - K0 + 1);                           // wave 0 is done with xr0 slot s % K0
      wait_word(pw + 64 * (NW - 1), seen_wl, s + ZA - LAP_ZL + 1);  // the last wave with zring's old record
      uint8_t *dst = xr0 + (s & (K0 - 1)) * SLOT + lane * REC_BYTES;
      const bool yreal = s + YOFF < T_above;
      const bool ywrite = !(U4K && !FACES) || yin;  // else xr0 holds the prefilled y = 0 face
      if (ywrite) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
          uint4 v = yreal ? make_uint4((uint32_t)f.y[2 * i], (uint32_t)(f.y[2 * i] >> 32),
                                       (uint32_t)f.y[2 * i + 1], (uint32_t)(f.y[2 * i + 1] >> 32))
                          : make_uint4(0u, 0u, 0u, 0u);
          if constexpr (LIT) {
            if (!yin) v = yface_lit(s, i);
          }
          if constexpr (VS) {
            if (!yin) v = yface_vs(s);
          }
          lds_write16(dst + i * PAIR, v);
        }
      }
      put_z(rz, f);
      lds_publish(pw + 64 * NW, s + 1, lane);  // wave 0 may run step s
      fetch(s + LPD, f, !PTHIN || (PHL + LPD) % LU == 0);
    };
    int32_t s = 0;
#pragma unroll 1
    for (; s + LU <= T; s += LU)
      static_for<0, LU>([&](auto ph) { LAP_INLINE(lstep(ph, s + decltype(ph)::value)); });
    static_for<0, LU>([&](auto ph) {
      if (s + decltype(ph)::value < T) LAP_INLINE(lstep(ph, s + decltype(ph)::value));
    });
    if (lane == 0) w_stall[0] = (int32_t)stalls;
  } else {
    // =================== compute waves ===================
    // a[i] of this lane at step t = sA2[t - 2w - (M lane + i) + OFF]
    const uint32_t a_lane = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)sA2 +
                            4u * (uint32_t)(OFF - 2 * w - M * lane - (M - 1));
    const int32_t y0 = L * RW + 2 * w;  // rows y0 (lo) and y0 + 1 (hi), 0-based
    const uint32_t bw = (y0 < lb ? SYM0 << tsa_sym(seqs, o1 + y0, pa.packed) : 0u) |
                        ((y0 + 1 < lb ? SYM0 << tsa_sym(seqs, o1 + y0 + 1, pa.packed) : 0u) << 16);
    uint32_t bv[M], c[M], SBC[M], K_[M], DMC[M], DMB[M];
    uint32_t oIx[M], shIz[M], svIxy[M], svIyz[M], shIxz[2][M], svM[2][M];
    uint32_t pIy[M], pIxy[M], pIyz[M], pBest[M];  // this wave's record of the previous step
    {
      uint32_t one1 = 0x00010001u, sbcv = pa.h_sbc, kdv = pa.h_kd, k0v = pa.h_k0;
      uint32_t dmb = 0u;
      if constexpr (VS) {
        // the [a=b] terms multiply b's one-hot code itself (a & b, no min):
        // DMB = dm / code(b) and, RTL s3, K = (d0 + [b=c] d1) / code(b)
        // (cell_messages_vs); both rows of the wave, one per half
        dmb = dm_over_code(pa.dmf, bw);
        if constexpr (!SOP) {
          k0v = dm_over_code(pa.d0f, bw);
          const uint32_t kb1 = dm_over_code(pa.d0f + pa.d1f, bw);
          kdv = (((kb1 & 0xFFFFu) - (k0v & 0xFFFFu)) & 0xFFFFu) | ((((kb1 >> 16) - (k0v >> 16)) & 0xFFFFu) << 16);
        }
      }
      asm volatile("" : "+v"(one1), "+v"(sbcv), "+v"(kdv), "+v"(k0v));
      const int64_t oc = o2 + (int64_t)q * ZT;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int k = M * lane + i;
        c[i] = (k < zt_q ? SYM0 << tsa_sym(seqs, oc + k, pa.packed) : 0u) * 0x00010001u;
        DMC[i] = dm_over_code(pa.dmf, c[i]);
        bv[i] = bw;
        const uint32_t e01 = pk_eq1(bw, c[i], one1);
        SBC[i] = pk_mad(e01, sbcv, 0u);
        K_[i] = pk_mad(e01, kdv, k0v);
        DMB[i] = dmb;
        oIx[i] = shIz[i] = pa.f_single;
        shIxz[0][i] = shIxz[1][i] = svIxy[i] = svIyz[i] = pa.f_pair;
        svM[0][i] = svM[1][i] = 0;
        pIy[i] = pIxy[i] = pIyz[i] = pBest[i] = 0;
      }
    }
    // LIT: the successors' symbols b_{y+1} (per half) and c_{z+1} (per position),
    // the per-position pair score of (y+1, z+1) less GE and the [b=c] part of
    // s3; the launch passes f_single = f_pair = 0, so the x' = 0 face column's
    // forced inputs and the initial states are zeros
    uint32_t bn = 0, cnl[M], UYZ[M], K1[M], lones = 0x00010001u;
    LitArgs cv = lit;
    if constexpr (LIT) {
      asm volatile("" : "+v"(lones), "+v"(cv.dmS), "+v"(cv.mmE), "+v"(cv.neS));
      bn = (y0 + 1 < lb ? SYM0 << tsa_sym(seqs, o1 + y0 + 1, pa.packed) : 0u) |
           ((y0 + 2 < lb ? SYM0 << tsa_sym(seqs, o1 + y0 + 2, pa.packed) : 0u) << 16);
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int32_t z1 = q * ZT + M * lane + i + 1;
        cnl[i] = (z1 < lc ? SYM0 << tsa_sym(seqs, o2 + z1, pa.packed) : 0u) * 0x00010001u;
        const uint32_t ebc = pk_eq1(bn, cnl[i], lones);
        UYZ[i] = pk_mad(ebc, cv.dmS, cv.mmE);
        K1[i] = SOP ? pk_mad(ebc, cv.dmS, lit.mm3S) : pk_mad(ebc, lit.d1S, lit.d0S);
      }
    }
    // CHK: halves of real cells (row y < lb, position z < LC of the tile); the
    // rest is masked to 0, a value the monitor's range contains anyway (faces)
    uint32_t vmask[M], vmax[M], vmin[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const uint32_t rowm = (y0 < lb ? 0x0000FFFFu : 0u) | (y0 + 1 < lb ? 0xFFFF0000u : 0u);
      vmask[i] = M * lane + i < zt_q ? rowm : 0u;
      vmax[i] = vmin[i] = 0u;
    }
    // END: no key yet; under pa.end_face only the row y = lb and the position
    // z = lc are candidates before x = la
    LapEndKeys<M, END> ek;
    if constexpr (END) {
      ek.kb = 2 * w + M * lane;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool on_face = y0 + h == lb - 1 || q * ZT + M * lane + i == lc - 1;
          ek.v[h][i] = 0u;
          ek.xlo[h][i] = (pa.end_face && !on_face) ? la - 1 : 0;
        }
    }
    uint32_t Q = F16 ? 0x08000800u : 0x00010001u, fsv = pa.f_single, fpv = pa.f_pair;
    uint32_t mlo = 0x0000FFFFu, mhi = 0xFFFF0000u;
    asm volatile("" : "+v"(Q), "+v"(fsv), "+v"(fpv), "+v"(mlo), "+v"(mhi));
    const PencilArgs pv = F16 ? pa : pin_score_consts(pa);
    const uint32_t sel0 = lane == 0 ? 0x03020100u : 0x07060504u;  // lane 0: whole word from the face
    // VS: the x = 0 face at the x = 1 cells of step t -- the low half's
    // position t - 2w and the high half's one behind share x + y + z =
    // t + L RW + zoff + 3, so one value for both: lam (t + L RW + zoff + 1)
    // for Ix, Ixy, Ixz (one lam less for M: the previous step's)
    uint32_t hx_cur = 0u, hx_prev = 0u;
    if constexpr (VS) {
      hx_cur = lam_bits(pa.lam, L * RW + q * ZT + 1);
      hx_prev = lam_bits(pa.lam, L * RW + q * ZT);
    }
    __syncthreads();  // the loader's prologue z records are in LDS
    if (zin || FACES) {  // position 0 before step 0 (tools/lap_emu.py: the same initial shifts)
      const uint8_t *r1 = zring + ((ZT - 1) & (LAP_ZL - 1)) * ZREC + w * LAP_ZREC_WAVE;
      const uint8_t *r2 = zring + ((ZT - 2) & (LAP_ZL - 1)) * ZREC + w * LAP_ZREC_WAVE;
      const uint4 a0 = lds_read16(r1), a1 = lds_read16(r1 + 16);
      const uint4 b0 = lds_read16(r2), b1 = lds_read16(r2 + 16);
      if (lane == 0) {
        shIz[0] = a0.x;
        svIyz[0] = a1.x;
        shIxz[1][0] = a0.z;
        svM[1][0] = a1.z;
        shIxz[0][0] = b0.z;
        svM[0][0] = b1.z;
      }
    }
    unsigned long long clk0 = 0;
    if (trace != nullptr) {
      stamp(1, now());
      clk0 = __builtin_amdgcn_s_memtime();  // shader clock: the loop's cycles (slot 6)
    }
    // wave 0's y input: xr0 slot t % K0, or the face record (stride 0)
    // (LIT / VS: always the loader's, which writes the step-varying faces)
    // (U4K: always xr0, which then holds the prefilled face)
    const bool yring = U4K || yin || FACES, zring_in = U4K || zin || FACES;
    const uint8_t *const ysrc = (yring ? xr0 : yface) + lane * REC_BYTES;
    const int32_t ystride = yring ? SLOT : 0;
    // position 0's z input: zring slot (t + ZT) % ZL = t % ZL, or the face record
    static_assert(ZT % LAP_ZL == 0, "z slot of step t: t % LAP_ZL");
    const uint8_t *const zsrc = (zring_in ? zring : zface) + w * LAP_ZREC_WAVE;
    const int32_t zstride = zring_in ? ZREC : 0;
    uint32_t a_nx[M];
    load_a<M>(a_lane, a_nx);
    uint32_t a_pair = a_lane;  // TSA_LAP_LEAN: a_lane's entry of the step pair's first step
    // U4K: the bases of the current group of four steps (t0 = t & ~3)
    uint32_t a_grp = a_lane;
    const uint8_t *y_grp = ysrc, *z_grp = zsrc;
    uint8_t *zst_grp = nullptr, *yst_grp = nullptr;
    // VBK: three VGPR bases (see the knob) -- v_rw: this lane's
    // record in the ring read (slot 0; wave 0: the ring it writes), the ring
    // written K slots above it; v_pwb: this lane's copy of the progress word
    // of wave w - 1 (wave 0: its own), the others at constant offsets above
    // it (every lane holds a copy, so a per-lane address reads the same
    // value); vlane: the SGPR-base stores' offset (the z record, stored by lane
    // 63, from a base 63 records lower)
    lds_u8 *v_rw = to_lds(xr + (w > 0 ? (w - 1) * K * SLOT : 0) + lane * REC_BYTES);
    lds_u8 *v_pwb = to_lds((uint8_t *)(pw + 64 * (w > 0 ? w - 1 : 0) + lane));
    // byte offsets from v_pwb: the input word (wave 0: the loader's), the own, the successor's
    auto pw_in = [](auto role) { return decltype(role)::value == 0 ? 4 * 64 * NW : 0; };
    auto pw_own = [](auto role) { return decltype(role)::value == 0 ? 0 : 4 * 64; };
    constexpr int WR_OFF = K * SLOT;  // v_rw + WR_OFF: the ring written (waves 1 ..)
    const lds_u8 *vy_grp = to_lds((uint8_t *)ysrc), *vz_grp = to_lds((uint8_t *)zsrc);
    const uint8_t *zst_s = zf_mine, *yst_s = yf_mine;  // SGPR bases of the group's ring records
    uint32_t vlane = (uint32_t)lane * REC_BYTES;
    if constexpr (VBK) asm volatile("" : "+v"(v_rw), "+v"(v_pwb), "+v"(vlane));
    auto set_group = [&](int32_t t0) {
      a_grp = a_lane + 4u * (uint32_t)t0;
      y_grp = ysrc + (t0 & (K0 - 1)) * SLOT;
      z_grp = zsrc + (t0 & (LAP_ZL - 1)) * ZREC;
      zst_grp = zf_mine + (int64_t)(t0 & (ZRm - 1)) * ZREC + w * LAP_ZREC_WAVE;
      yst_grp = yf_mine + (int64_t)(t0 & (YRm - 1)) * SLOT + lane * REC_BYTES;
      if constexpr (VBK) {
        vy_grp = to_lds((uint8_t *)y_grp);
        vz_grp = to_lds((uint8_t *)z_grp);
        asm volatile("" : "+v"(vy_grp), "+v"(vz_grp));
        zst_s = (const uint8_t *)sgpr64((uint64_t)(uintptr_t)(zf_mine + (int64_t)(t0 & (ZRm - 1)) * ZREC +
                                                              w * LAP_ZREC_WAVE - 63 * REC_BYTES));
        yst_s = (const uint8_t *)sgpr64((uint64_t)(uintptr_t)(yf_mine + (int64_t)(t0 & (YRm - 1)) * SLOT));
      }
    };
    // producer side: my consumers' progress (y: the lap below, via the last
    // wave; z: the tile to the right, every wave), LDS-DMA'd by the loader
    int32_t seen_in = 0, seen_out = 0, seen_y = 0, seen_z = 0;
    uint32_t n_bp = 0;
#if defined(TSA_DIAG)  // shader cycles: reads + pre-cell, check, post + stores, step gap
    uint64_t prof[4] = {0, 0, 0, 0}, prof_last = 0;
    int32_t lag_y = 0, lag_z = 0;  // t - the consumer's progress, at the ring stores
#endif
    constexpr int LM = M == 1 ? 0 : M == 2 ? 1 : M == 4 ? 2 : 3;  // log2 M
    int32_t klo = -2 * w, ihi = 0;  // x = 1 position of the low half at the current step
    uint64_t lm_hi = 0;             // the high half's lane mask (previous step's low)
    auto prog_decode = [&](int32_t v) -> int32_t {
      return ((uint32_t)v >> 13) == ep19 ? (int32_t)(v & 0x1FFF) : 0;
    };
    auto wait_consumer = [&](int64_t cons, int32_t &seen, int32_t *word, int32_t need) {
      if (need <= seen) return;
      seen = max(seen, prog_decode(lds_word(word)));
      if (need <= seen) return;
      ++n_bp;
      for (uint32_t spin = 0;; ++spin) {
        const int32_t v = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(prog + cons * LAP_PROG_STRIDE, __ATOMIC_RELAXED, SCOPE));
        seen = max(seen, prog_decode(v));
        if (need <= seen) return;
        if (spin >= spin_limit || timed_out || ((spin & 63) == 63 && lds_word(w_abort) != 0)) {
          fail();
          seen = 1 << 24;
          return;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    };
    const int64_t cons_y = yout ? lid + GZ : -1, cons_z = zout ? lid + 1 : -1;
    // Room in my z ring for record tt: the consumer's loader checks record
    // s + ZT + ZA at its step s, so a published progress p covers records up
    // to p - 1 + ZT + ZA -- and its prologue reads ZT - 2 .. ZT + ZA - 1
    // before it publishes anything, so overwriting one of those (or later)
    // needs p >= 1 even where that formula gives <= 0: a consumer that starts
    // late (its physical workgroup still on a lap of the previous round) would
    // otherwise find its prologue records overwritten and wait forever
    auto z_need = [&](int32_t tt) -> int32_t {
      const int32_t r = tt - ZRm;  // the record slot tt & (ZRm - 1) holds before
      return r >= ZT - 2 ? max(1, r - ZT - ZA + 1) : 0;
    };

    // ROLE: 0 = wave 0, 1 = middle waves, 2 = the last wave (NW >= 2)
    // QS: t & 3 in a four-step group (addresses at constant offsets from the
    // group's bases), -1: addresses from t
    auto step = [&](auto ph, auto role, int32_t t, auto fin_step, auto qs) {
      constexpr int PH = decltype(ph)::value;
      constexpr int ROLE = decltype(role)::value;
      constexpr bool FIN = decltype(fin_step)::value;
      constexpr int QS = decltype(qs)::value;
      uint32_t a[M];
#pragma unroll
      for (int i = 0; i < M; ++i) a[i] = a_nx[i];
      if constexpr (QS >= 0) load_a_off<M>(a_grp, QS + 1, a_nx);
      else if constexpr (TSA_LAP_LEAN) load_a_off<M>(a_pair, PH + 1, a_nx);  // entry t + 1 of a_lane's table
      else load_a<M>(a_lane + 4u * (uint32_t)(t + 1), a_nx);
      // ---- input reads, issued first: the producer's progress word (unless the
      // cached value covers step t), then its record. LDS executes a wave's DS
      // instructions in order, so a word read that covers t proves the record
      // read behind it current; the check waits until the pre-cell is done.
#if defined(TSA_DIAG)
      const uint64_t pt0 = __builtin_amdgcn_s_memtime();
#endif
      const int32_t need = ROLE == 0 ? t + 1 : t;
      const int32_t *const pword = ROLE == 0 ? pw + 64 * NW : pw + 64 * (w - 1);
      const bool waits = ROLE != 0 || yin || zin || FACES;
      const bool poll = TSA_LAP_LEAN ? waits : (waits && seen_in < need);
      int32_t fl_v = 0;
      constexpr bool VB = QS >= 0 && VBK;  // this step's accesses off the VGPR bases
      if (poll) {
        if constexpr (VB)
          fl_v = *(volatile const __attribute__((address_space(3))) int32_t *)(v_pwb + pw_in(role));
        else
          fl_v = *(volatile const __attribute__((address_space(3))) int32_t *)(
              const __attribute__((address_space(3))) void *)pword;
      }
      asm volatile("" ::: "memory");
      const uint8_t *src = QS >= 0 ? (ROLE == 0 ? y_grp + QS * SLOT
                                                : xr + ((w - 1) * K + ((QS + K - 1) & (K - 1))) * SLOT + lane * REC_BYTES)
                         : ROLE == 0 ? ysrc + (t & (K0 - 1)) * ystride
                                     : xr + ((w - 1) * K + ((t - 1) & (K - 1))) * SLOT + lane * REC_BYTES;
      const lds_u8 *srcl = VB ? (ROLE == 0 ? vy_grp + (VB ? QS : 0) * SLOT
                                           : v_rw + (((VB ? QS : 0) + K - 1) & (K - 1)) * SLOT)
                              : to_lds((uint8_t *)src);
      uint4 rv[M];
      auto read_rec = [&]() {
#pragma unroll
        for (int i = 0; i < M; ++i) {
          if constexpr (ROLE == 0 && TSA_LAP_Y2) {  // {payload, tag, payload, tag}: the payloads only
            const __attribute__((address_space(3))) uint32_t *p =
                (const __attribute__((address_space(3))) uint32_t *)(srcl + i * PAIR);
            rv[i] = make_uint4(p[0], 0u, p[2], 0u);
          } else {
            rv[i] = lds_read16_at(srcl, i * PAIR);
          }
        }
      };
      read_rec();
      // the successor's progress, read now and consulted before the record store
      // (TSA_LAP_GCHK groups, K = 4: on even steps only, covering the next step too)
      constexpr bool SUCC_HERE = !(QS >= 0 && TSA_LAP_GCHK && K == 4) || (QS & 1) == 0;
      int32_t succ_v = 0;
      if constexpr (ROLE != 2 && SUCC_HERE && VB)
        succ_v = *(volatile const __attribute__((address_space(3))) int32_t *)(v_pwb + pw_own(role) + 4 * 64);
      else if constexpr (ROLE != 2 && SUCC_HERE)
        succ_v = *(volatile const __attribute__((address_space(3))) int32_t *)(
            const __attribute__((address_space(3))) void *)(pw + 64 * (w + 1));
      // position 0's z-1 neighbour for the next step: the z = 0 face, or the
      // left tile's record t + ZT (checked by the loader: see ZA)
      // (four 4-byte reads, merged into two ds_read2_b32: reading the tags too
      // hands the compiler dead registers it reuses, forcing lgkmcnt(0) waits)
      const uint8_t *zr = QS >= 0 ? z_grp + QS * ZREC : zsrc + ((t + ZT) & (LAP_ZL - 1)) * zstride;
      const lds_u8 *zrl = VB ? vz_grp + (VB ? QS : 0) * ZREC : to_lds((uint8_t *)zr);
      auto lds32 = [](const lds_u8 *p) { return *(const __attribute__((address_space(3))) uint32_t *)p; };
      const uint32_t fIz = lds32(zrl), fIxz = lds32(zrl + 8), fIyz = lds32(zrl + 16), fM = lds32(zrl + 24);
      uint32_t inIx[M], inIz[M], inIxy[M], inIyz[M], inIxz[M], inM[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        inIx[i] = oIx[i];
        inIz[i] = shIz[i];
        inIxy[i] = svIxy[i];
        inIyz[i] = svIyz[i];
        inIxz[i] = shIxz[PH][i];
        inM[i] = svM[PH][i];
      }
      // ---- x = 1: low half at position klo = t - 2w, high half one position
      // behind (= the low half's position of the previous step); their x - 1
      // inputs are the x = 0 face (src/PE_1cyc.v:164-178,196-218). Branch-free:
      // SALU lane masks (zero outside the tile) and one bfi mask per register.
      const uint64_t lm_lo = lane_bit(klo >> LM);
      const int32_t ilo = klo & (M - 1);
      uint32_t mx[M];  // LIT: the x' = 0 halves, whose Y is forced to 0 as it lands
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const uint64_t ml = (M == 1 || ilo == i) ? lm_lo : 0ull;
        const uint64_t mh = (M == 1 || ihi == i) ? lm_hi : 0ull;
        uint32_t m0, m1;
        asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(m0) : "v"(mhi), "s"(mh));
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(m1) : "v"(m0), "v"(mlo), "s"(ml));
        inIx[i] = vbfi(m1, VS ? hx_cur : fsv, inIx[i]);
        inIxy[i] = vbfi(m1, VS ? hx_cur : fpv, inIxy[i]);
        inIxz[i] = vbfi(m1, VS ? hx_cur : fpv, inIxz[i]);
        inM[i] = vbfi(m1, VS ? hx_prev : 0u, inM[i]);
        if constexpr (LIT) {
          inIz[i] = vbfi(m1, 0u, inIz[i]);
          inIyz[i] = vbfi(m1, 0u, inIyz[i]);
          mx[i] = m1;
        }
      }
      if constexpr (VS) {
        hx_prev = hx_cur;
        hx_cur = U(H(hx_cur) + H(pa.v_lam));
      }
      lm_hi = lm_lo;
      ihi = ilo;
      ++klo;
      // ---- the cell, up to the row above
      LapPre<M> pre;
      LitPre<M> lpre;
      if constexpr (LIT)
        lit_pre<M, SOP>(lit, cv, lones, a, bn, cnl, UYZ, K1, inIx, inIz, inIxy, inIyz, inIxz, inM, lpre);
      else if constexpr (VS)
        lap_pre_vs<M, SOP>(a, bv, c, SBC, K_, DMC, DMB, pa, inIx, inIz, inIxy, inIyz, inIxz, inM, pre);
      else if constexpr (F16)
        lap_pre_f16<M, SOP>(a, bv, c, SBC, K_, DMC, Q, pa, inIx, inIz, inIxy, inIyz, inIxz, inM, pre);
      else
        lap_pre_i16<M, SOP>(a, bv, c, Q, pv, inIx, inIz, inIxy, inIyz, inIxz, inM, pre);
      // pin the pre-cell here: left alone the compiler sinks it below the
      // progress check, so the record read's latency would not be covered
#pragma unroll
      for (int i = 0; i < M; ++i) {
        if constexpr (LIT) {
          asm volatile("" : "+v"(lpre.pIx[i]), "+v"(lpre.pIy[i]), "+v"(lpre.pIz[i]), "+v"(lpre.pIxy[i]),
                       "+v"(lpre.pIyz[i]), "+v"(lpre.pIxz[i]), "+v"(lpre.pM[i]));
          asm volatile("" : "+v"(lpre.uxy[i]), "+v"(lpre.vxz[i]), "+v"(lpre.s3[i]));
        } else {
          asm volatile("" : "+v"(pre.W[i]), "+v"(pre.N1[i]), "+v"(pre.N2[i]), "+v"(pre.N3[i]),
                       "+v"(pre.N4[i]), "+v"(pre.N5[i]), "+v"(pre.N6[i]));
        }
      }
#if defined(TSA_DIAG)
      const uint64_t pt1 = __builtin_amdgcn_s_memtime();
#endif
      // ---- the input record is current? (slow path: poll, then read it again)
      if (poll) {
        seen_in = max(seen_in, (int32_t)__builtin_amdgcn_readfirstlane(fl_v));
        if (seen_in < need) {
          wait_word(pword, seen_in, need);
          asm volatile("" ::: "memory");
          read_rec();
        }
      }
      // ---- the row above of both halves
      uint32_t Ry[M], Rxy[M], Ryz[M], Rb[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        if constexpr (ROLE != 0) {  // wave w-1's high halves
          Ry[i] = rows2(pIy[i], rv[i].x);
          Rxy[i] = rows2(pIxy[i], rv[i].y);
          Ryz[i] = rows2(pIyz[i], rv[i].z);
          Rb[i] = rows2(pBest[i], rv[i].w);
        } else {  // tagged record {Iy.hi | Ixy.hi << 16, tag, Iyz.hi | best.hi << 16, tag}
          Ry[i] = perm(pIy[i], rv[i].x, 0x05040100u);
          Rxy[i] = perm(pIxy[i], rv[i].x, 0x05040302u);
          Ryz[i] = perm(pIyz[i], rv[i].z, 0x05040100u);
          Rb[i] = perm(pBest[i], rv[i].z, 0x05040302u);
        }
      }
#if defined(TSA_DIAG)
      asm volatile("" :: "v"(Ry[0]));
      const uint64_t pt2 = __builtin_amdgcn_s_memtime();
#endif
      uint32_t oIy[M], oIxy[M], oIyz[M], oBest[M], oIz[M], oIxz[M], nIx[M];
      if constexpr (LIT) {  // (oBest: the push into M, the record's fourth word)
#pragma unroll
        for (int i = 0; i < M; ++i) Ry[i] = vbfi(mx[i], 0u, Ry[i]);
        lit_post<M>(lit, Ry, UYZ, lpre, nIx, oIy, oIz, oIxy, oIyz, oIxz, oBest);
      } else if constexpr (VS) {
        lap_post_vs<M>(pa, Ry, pre, nIx, oIy, oIz, oIxy, oIyz, oIxz, oBest);
      } else if constexpr (F16) {
        lap_post_f16<M>(pa, Ry, pre, nIx, oIy, oIz, oIxy, oIyz, oIxz, oBest);
      } else {
        lap_post_i16<M>(pv, Ry, pre, nIx, oIy, oIz, oIxy, oIyz, oIxz, oBest);
      }
      if constexpr (CHK) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
          const uint32_t v = oBest[i] & vmask[i];
          vmax[i] = pk_max(vmax[i], v);
          vmin[i] = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(
                                                     __builtin_bit_cast(s16x2, vmin[i]),
                                                     __builtin_bit_cast(s16x2, v)));
        }
      }
      if constexpr (END) {  // x - 1 = t - (2w + h) - (M lane + i): a candidate inside [xlo, la - 1]
        const int32_t x0 = t - ek.kb, xhi = la - 1;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int32_t xm1 = x0 - (i + h);
            const bool cand = min(max(xm1, ek.xlo[h][i]), xhi) == xm1;
            const uint32_t val = (h ? (oBest[i] & 0xFFFF0000u) : (oBest[i] << 16)) ^ 0x80000000u;
            ek.v[h][i] = max(ek.v[h][i], cand ? (val | (uint32_t)(0xFFFF - xm1)) : 0u);
          }
        }
      }
      if constexpr (FIN && !END) {  // the final cell (src/TriAlign_1cyc.v:141-142,342-345)
        if (final_wg && w == (r_f >> 1)) {  // row r_f: half r_f & 1 of wave r_f / 2
#pragma unroll
          for (int i = 0; i < M; ++i) {
            if constexpr (LIT) {  // the cell's 7 inputs {M, Ix, Iy, Iz, Ixy, Iyz, Ixz}
              fin[(0 * M + i) * 64 + lane] = inM[i];
              fin[(1 * M + i) * 64 + lane] = inIx[i];
              fin[(2 * M + i) * 64 + lane] = Ry[i];
              fin[(3 * M + i) * 64 + lane] = inIz[i];
              fin[(4 * M + i) * 64 + lane] = inIxy[i];
              fin[(5 * M + i) * 64 + lane] = inIyz[i];
              fin[(6 * M + i) * 64 + lane] = inIxz[i];
            } else {
              fin[i * 64 + lane] = oBest[i];
            }
          }
        }
      }
      // ---- records: to the wave below (LDS), or (last wave) the y ring
      if constexpr (ROLE != 2) {
        if constexpr (SUCC_HERE) {
          constexpr int AHEAD = (QS >= 0 && TSA_LAP_GCHK && K == 4) ? 1 : 0;
          seen_out = max(seen_out, (int32_t)__builtin_amdgcn_readfirstlane(succ_v));
          wait_word(pw + 64 * (w + 1), seen_out, t + AHEAD - K + 2);  // wave w+1 read slot t % K's old record
        }
        uint8_t *dst = xr + (w * K + ((QS >= 0 ? QS : t) & (K - 1))) * SLOT + lane * REC_BYTES;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          const uint4 v = make_uint4(oIy[i], oIxy[i], oIyz[i], oBest[i]);
          if constexpr (VB) lds_write16_at(v_rw, (ROLE == 0 ? 0 : WR_OFF) + ((VB ? QS : 0) & (K - 1)) * SLOT + i * PAIR, v);
          else lds_write16(dst + i * PAIR, v);
        }
      } else {
        if (yout) {
#if defined(TSA_DIAG)
          lag_y = max(lag_y, t - prog_decode(lds_word(bpw)));
#endif
          // (TSA_LAP_GCHK groups: once per group, for its last step)
          if (!(QS >= 0 && TSA_LAP_GCHK)) wait_consumer(cons_y, seen_y, bpw, t - YRm - YOFF + 1);
          else if (QS == 0) wait_consumer(cons_y, seen_y, bpw, t + 3 - YRm - YOFF + 1);
          const uint32_t tg = lap_tag(epoch, t);
          static_for<0, M>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            const uint4 v = make_uint4(perm(oIxy[i], oIy[i], 0x07060302u), tg,
                                       perm(oBest[i], oIyz[i], 0x07060302u), tg);
            constexpr int OFFB = (QS * M + i) * PAIR;
            if constexpr (VB && OFFB < 4096) store16_sc1_s<SYS, (VB ? OFFB : 0)>(yst_s, vlane, v);
            else if constexpr (QS >= 0 && OFFB < 4096) store16_sc1_at<SYS, OFFB>(yst_grp, v);
            else if constexpr (QS >= 0) store16_sc1<SYS>(yst_grp + OFFB, v);
            else store16_sc1<SYS>(yf_mine + ((int64_t)(t & (YRm - 1)) * M + i) * PAIR + lane * REC_BYTES, v);
          });
        }
        // my producers' back-pressure: the loader has checked at least
        // t - NW + 2 steps (wave 0 ran t - NW + 1 before this wave's step t)
        const bool pub_step = (QS >= 0 && LAP_PUB == 4) ? QS == 0 : (t & (LAP_PUB - 1)) == 0;
        if ((yin || zin) && pub_step && lane == 0)
        {
          const int32_t pv_ = (int32_t)((ep19 << 13) | (uint32_t)max(t - NW + 2, 0));
          __hip_atomic_store(prog + lid * LAP_PROG_STRIDE, pv_, __ATOMIC_RELAXED, SCOPE);
          if constexpr (SYS) {
            if (prog_x != nullptr) __hip_atomic_store(prog_x, pv_, __ATOMIC_RELAXED, SCOPE);
          }
        }
      }
      // ---- z record of this wave's last position (lane 63, register M-1)
      if (zout) {
#if defined(TSA_DIAG)
        lag_z = max(lag_z, t - prog_decode(lds_word(bpw + 1)));
#endif
        if (!(QS >= 0 && TSA_LAP_GCHK)) wait_consumer(cons_z, seen_z, bpw + 1, z_need(t));
        else if (QS == 0) wait_consumer(cons_z, seen_z, bpw + 1, z_need(t + 3));
        if (lane == 63) {
          const uint32_t tg = lap_tag(epoch, t);
          if constexpr (VB) {
            store16_sc1_s<SYS, (VB ? QS : 0) * ZREC>(zst_s, vlane, make_uint4(oIz[M - 1], tg, oIxz[M - 1], tg));
            store16_sc1_s<SYS, (VB ? QS : 0) * ZREC + 16>(zst_s, vlane, make_uint4(Ryz[M - 1], tg, Rb[M - 1], tg));
          } else if constexpr (QS >= 0) {
            store16_sc1_at<SYS, (QS >= 0 ? QS : 0) * ZREC>(zst_grp, make_uint4(oIz[M - 1], tg, oIxz[M - 1], tg));
            store16_sc1_at<SYS, (QS >= 0 ? QS : 0) * ZREC + 16>(zst_grp, make_uint4(Ryz[M - 1], tg, Rb[M - 1], tg));
          } else {
            uint8_t *zdst = zf_mine + (int64_t)(t & (ZRm - 1)) * ZREC + w * LAP_ZREC_WAVE;
            store16_sc1<SYS>(zdst, make_uint4(oIz[M - 1], tg, oIxz[M - 1], tg));
            store16_sc1<SYS>(zdst + 16, make_uint4(Ryz[M - 1], tg, Rb[M - 1], tg));
          }
        }
      }
      if constexpr (VB) {  // lds_publish through the base
        asm volatile("" ::: "memory");
        *(volatile __attribute__((address_space(3))) int32_t *)(v_pwb + pw_own(role)) = t + 1;
        asm volatile("" ::: "memory");
      } else {
        lds_publish(pw + 64 * w, t + 1, lane);
      }
#if defined(TSA_DIAG)
      const uint64_t pt3 = __builtin_amdgcn_s_memtime();
      prof[0] += pt1 - pt0;
      prof[1] += pt2 - pt1;
      prof[2] += pt3 - pt2;
      prof[3] += prof_last ? pt0 - prof_last : 0;
      prof_last = pt3;
#endif
      // ---- advance the systolic registers
#pragma unroll
      for (int i = 0; i < M; ++i) {
        oIx[i] = nIx[i];
        svIxy[i] = Rxy[i];
        pIy[i] = oIy[i];
        pIxy[i] = oIxy[i];
        pIyz[i] = oIyz[i];
        pBest[i] = oBest[i];
      }
      zshift<M>(shIxz[PH], oIxz, sel0, fIxz);
      zshift<M>(shIz, oIz, sel0, fIz);
      zshift<M>(svIyz, Ryz, sel0, fIyz);
      zshift<M>(svM[PH], Rb, sel0, fM);
    };
    auto run = [&](auto role) {  // the last step peeled off (it records the final cell)
      int32_t t = 0;
      const int32_t T1 = T - 1;
      constexpr std::integral_constant<int, 0> P0{};
      constexpr std::integral_constant<int, 1> P1{};
      constexpr std::false_type mid{};
      constexpr std::true_type last{};
      constexpr std::integral_constant<int, -1> QD{};
      if constexpr (U4K) {
        constexpr std::integral_constant<int, 0> Q0{};
        constexpr std::integral_constant<int, 1> Q1{};
        constexpr std::integral_constant<int, 2> Q2{};
        constexpr std::integral_constant<int, 3> Q3{};
#pragma unroll 1
        for (; t + 3 < T1; t += 4) {
          set_group(t);
          LAP_INLINE(step(P0, role, t, mid, Q0));
          LAP_INLINE(step(P1, role, t + 1, mid, Q1));
          LAP_INLINE(step(P0, role, t + 2, mid, Q2));
          LAP_INLINE(step(P1, role, t + 3, mid, Q3));
        }
      }
#pragma unroll 1
      for (; t + 1 < T1; t += 2) {
        a_pair = a_lane + 4u * (uint32_t)t;
        LAP_INLINE(step(P0, role, t, mid, QD));
        LAP_INLINE(step(P1, role, t + 1, mid, QD));
      }
      a_pair = a_lane + 4u * (uint32_t)t;
      if (t < T1) {
        LAP_INLINE(step(P0, role, t, mid, QD));
        LAP_INLINE(step(P1, role, t + 1, last, QD));
      } else {
        LAP_INLINE(step(P0, role, t, last, QD));
      }
    };
    static_assert(NW >= 2, "wave 0 and the last wave are distinct roles");
    if (w == 0) LAP_INLINE(run(std::integral_constant<int, 0>{}));
    else if (w == NW - 1) LAP_INLINE(run(std::integral_constant<int, 2>{}));
    else LAP_INLINE(run(std::integral_constant<int, 1>{}));
    if (trace != nullptr) {
      const unsigned long long clk1 = __builtin_amdgcn_s_memtime();
      stamp(2, now());
      if (tid == 0) {
        trace[(int64_t)b * LAP_TRACE_SLOTS + 5] = n_wait;
        trace[(int64_t)b * LAP_TRACE_SLOTS + 6] = clk1 - clk0;
      }
    }
    if (w == NW - 1 && lane == 0) w_bp[0] = (int32_t)n_bp;
    if constexpr (CHK) {  // the wave's extremes -> the triple's monitor words
      int32_t mx = 0, mn = 0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int32_t lo0 = (int16_t)(vmax[i] & 0xFFFF), hi0 = (int16_t)(vmax[i] >> 16);
        const int32_t lo1 = (int16_t)(vmin[i] & 0xFFFF), hi1 = (int16_t)(vmin[i] >> 16);
        mx = max(mx, max(lo0, hi0));
        mn = min(mn, min(lo1, hi1));
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        mx = max(mx, __shfl_xor(mx, d));
        mn = min(mn, __shfl_xor(mn, d));
      }
      if (lane == 0) {
        if constexpr (TSA_CHK_SLOTS) {  // this wave's slot of [max] NC G NW, [min] NC G NW
          const int64_t nslot = (int64_t)NC * G * NW;
          mon[lid * NW + w] = mx;
          mon[nslot + lid * NW + w] = mn;
        } else {
          const int32_t ntri = NC / GZ;
          atomicMax(mon + tri, mx);
          atomicMin(mon + ntri + tri, mn);
        }
      }
    }
    if constexpr (END) {  // the wave's largest key {best : ~(x - 1)} : ~(y - 1) : ~(z - 1) -> its slot
      unsigned long long bk = 0ull;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int32_t yy = y0 + h, k = M * lane + i;  // 0-based row, tile position
          const unsigned long long k64 = ((unsigned long long)ek.v[h][i] << 32) |
                                         ((uint32_t)(0xFFFF - yy) << 16) | (uint32_t)(0xFFFF - (q * ZT + k));
          if (yy < lb && k < zt_q && ek.v[h][i] != 0u) bk = max(bk, k64);
        }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) bk = max(bk, (unsigned long long)__shfl_xor(bk, d));
      if (lane == 0) ekey_[lid * NW + w] = bk;
    }
#if defined(TSA_DIAG)
    if (trace != nullptr && lane == 0 && w < 8)
      for (int k = 0; k < 4; ++k) trace[(int64_t)b * LAP_TRACE_SLOTS + 8 + 4 * w + k] = prof[k];
    if (trace != nullptr && lane == 0) {
      atomicMax(trace + (int64_t)b * LAP_TRACE_SLOTS + 40, (unsigned long long)max(lag_y, 0));
      atomicMax(trace + (int64_t)b * LAP_TRACE_SLOTS + 41, (unsigned long long)max(lag_z, 0));
    }
#endif
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the final cell and the loader's counters are in LDS
  if (trace != nullptr && tid == 0) {
    trace[(int64_t)b * LAP_TRACE_SLOTS + 4] = (unsigned long long)w_stall[0];
    trace[(int64_t)b * LAP_TRACE_SLOTS + 7] = (unsigned long long)w_bp[0];
  }
  if constexpr (LIT) {
    if (final_wg) {  // block-uniform: the final cell's 7-tuple, unshifted, and its MAX7
      const int32_t kf = k_f, hf = r_f & 1;
      if (tid < 7) {
        const uint32_t v = fin[(tid * M + kf % M) * 64 + kf / M];
        fin[7 * M * 64 + tid] = (uint32_t)((int32_t)(int16_t)(uint16_t)(hf ? (v >> 16) : (v & 0xFFFF)) >> lit.sh);
      }
      __syncthreads();
      if (tid == 0) {
        const bool bad = __hip_atomic_load(err, __ATOMIC_RELAXED, SCOPE) == epoch;
        int32_t best = (int32_t)fin[7 * M * 64];
        for (int k = 1; k < 7; ++k) best = max(best, (int32_t)fin[7 * M * 64 + k]);
        scores[tri] = bad ? TSA_SCORE_INVALID : best;  // FINAL MAX7, src/TriAlign_1cyc.v:141-142
        if (mon != nullptr)
          for (int k = 0; k < 7; ++k) mon[7 * (int64_t)tri + k] = (int32_t)fin[7 * M * 64 + k];
      }
    }
  } else if (!END && final_wg && tid == 0) {  // (END: lap_ends_reduce writes the triple's score)
    const int32_t kf = k_f, hf = r_f & 1;
    const uint32_t v = fin[(kf % M) * 64 + kf / M];
    const uint16_t hb = (uint16_t)(hf ? (v >> 16) : (v & 0xFFFF));
    // a timed-out hand-off anywhere upstream invalidates the score (every
    // workgroup of the triple precedes this one): report it in-band
    const bool bad = __hip_atomic_load(err, __ATOMIC_RELAXED, SCOPE) == epoch;
    // VS: the final cell's value sits lam (la + lb + lc) above its score
    const int32_t vsh = VS ? pa.lam * (la + lb + lc) : 0;
    scores[tri] = bad ? TSA_SCORE_INVALID
                      : F16 ? (int32_t)(float)__builtin_bit_cast(_Float16, hb) - vsh : (int32_t)(int16_t)hb;
  }
  };
  const int32_t slots = (L1_ - L0_) * CH_, sx = rd_.SX;  // logical slots per XCD
  for (int32_t slot = (int32_t)(blockIdx.x >> 3); slot < slots; slot += sx) {
    lap_body(slot);
    __syncthreads();  // the next lap re-initialises this workgroup's LDS
  }
