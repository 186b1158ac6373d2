"""CPU replay of the helix kernel's schedule (csrc/pencil_kernel.hip).

TEST/DESIGN INFRASTRUCTURE: the helix's index and timing logic -- positions,
halves, the two-step wave skew, LDS record slots, the wave-0 ring with its
face rows, x = 1 injection, z-shifts with the z = 0 face, the final-cell
capture -- executed register by register with exact integer arithmetic, in
the message form (`vs=False`) or the V-space form of cell_messages_vs
(`vs=True`: values shifted by lam*(x+y+z), faces lam*q). tests/
test_pencil_schedule.py checks it against the oracle.

V-space replays the kernel's first-lap role too: wave 0 builds the y = 0 face
records of its steps before t_sw from its own H values, only the ring rows of
steps [t_sw, lag) are filled, and `ring_garbage_seed` starts the ring as
garbage, so a row read before it is written shows (tests/test_helix_ring_emu.py).

`shifted=True` (V-space only) models a record layout the kernel no longer has
(the writer-shifted records of DESIGN.md 4.2, retired after they measured
slower); it stays as an independent replay of the algebra against the oracle.
It replays the writer-side record shift: a wave (and the last wave, into the ring) stores
each position's {Iyz, best} at position k+1, lane 0's low halves carrying the
z = 0 face the READER needs -- the writer's own H(t+2) after its lap-wrap
update, which equals the reader's H(t'+1) two steps later (same u, one row
down) -- so the reader takes Iyz and M from its record with no z-shift.

`read_prev=True` (V-space, not `shifted`; the kernel's RP forms) replays
the reader-side address rule: a lane takes {Iyz, best} of the row above from
the RECORD of position k-1 -- register i-1 of its own lane, or register M-1 of
lane-1 (lane 63 for lane 0) for register 0 -- and only lane 0's register 0 is
fixed up after the read ({z = 0 face, lane 63's low half}). No write changes, so
wave 0 reads the ring rows the same way.
The emulator has no LDS addresses: this replays the DATA rule only (which
record's halves each lane and register ends up with), and gives what the
reader's z-shift gives. The kernel's address arithmetic -- the lane - 1 base,
the record offsets, wave 0's slot base -- is guarded by the GPU tests alone
(tests/test_helix_prev_reads.py).

`int_bits=True` (with `vs` and `read_prev`, M = 2; the kernel's integer-pattern
cell, cell_messages_vi) carries what the registers hold: every half is the
16-bit pattern u = bias + 8 V, a register the 32-bit word of its two halves.
The cell's constant adds and subtracts are done on the 32-bit word, the match
bonuses per half mod 2^16 (v_pk_mad_u16), every max on the halves as unsigned
16-bit integers; symbol codes are 1 << s and the per-row weights 8 w / code.
LDS and ring garbage are random 16-bit patterns. Two events are counted into
the `events` dict: "window", a half of a started position (t >= S w + k)
leaving [0x0400, 0x7BFF] after an operation of the cell, and "carry", an add or
subtract whose low half carried or borrowed while the high half beside it held
a started position. `bias` defaults to the host predicate's (vi_bias below, the
rule of use_vi in csrc/pencil_kernel.hip); the other modes are unchanged.

A caller that passes `events={"range": {}}` (message form or V-space form, not
`int_bits`) gets back in that dict the (min, max) of every intermediate the
halves holding a REAL cell (x <= LA, y <= LB, z <= LC, started) form at a step,
by group: "in" (the seven inputs of the cell, faces and injections included),
and for the message form "state" (the seven states), "term" (the 49 differences
S[s] - P[T][s]) and "msg" (the seven messages); for the V-space form "sum" (the
inputs plus their match bonuses), "max" (the group maxima, best, best - (GO -
GE), the pair messages) and "out" (the terms and results of the single-gap
messages). V-space values are shifted by lam (x + y + z). These are what
pencil_slack (csrc/pencil_kernel.hip) has to cover around the candidate range
(tests/test_range_proof.py). Without the key nothing is recorded.

`shared_fetch=True` (V-space with `read_prev`, M = 2; the kernel's RP forms)
replays who fetches wave 0's ring rows and when. Wave 0 reads
step t's row from slot t mod PD of its LDS ring copy (xr0) and issues nothing;
waves 1 and 2 issue at the first and the third step t of every four-step group,
from PD steps before t_sw on, the row of step t + 6 (wave 1) or t + 7 (wave 2)
into that step's slot. A slot is IN FLIGHT, its contents undefined, from the
step its fetch is issued until the issuing wave's counted wait (at the step
after an issue: all but its two newest rows have landed) and the barrier that
follows. The step barrier (after every odd step) is the only order between
waves, so two things in one barrier interval are unordered. Two events are
counted into `events`: "fetch_in_flight", wave 0 reading a slot that is in
flight or does not hold its step's row, and "fetch_unread", a fetch issued
into a slot whose row wave 0 has not read before the interval's opening
barrier (or that is itself still in flight). Either leaves garbage in the
record wave 0 reads. `fetch_shift=k` moves every fetch k barrier intervals
EARLIER (k < 0: later) than the kernel's schedule: the test hook that shows
both rules bite.

Layout as in the kernel: NW = 8 waves, wave w owns row y = lap*NW + w + 1;
lane l, register i, half h is position k = 64M h + M l + i (TWO mode, LC <= 64
and M = 1: k = l, and half h scores its own triple); position k of wave w
computes x = (t - S w - k) mod P + 1 at step t (S = 2).
"""
from __future__ import annotations

import numpy as np

NW, S, RING_EXTRA, PD = 8, 2, 8, 8
FILL_FROM = 0  # test hook: the first rows wave 0 fetches left unfilled (the garbage ring must then show)


def penalties(go, ge):
    GO2, GE2, GOGE = 2 * go, 2 * ge, go + ge
    return np.array([[0, 0, 0, 0, 0, 0, 0],
                     [GO2, GE2, GOGE, GOGE, GOGE, GO2, GOGE],
                     [GO2, GOGE, GE2, GOGE, GOGE, GOGE, GO2],
                     [GO2, GOGE, GOGE, GE2, GO2, GOGE, GOGE],
                     [go, ge, ge, go, ge, go, go],
                     [go, go, ge, ge, go, ge, go],
                     [go, ge, go, ge, go, go, ge]], dtype=np.int64)


VI_LO, VI_HI = 0x0400, 0x7BFF


def value_bound(la, lb, lc, match, mismatch, go, ge, sop):
    """csrc/trialign_api.hip value_bound: [lo, hi] of every state and candidate."""
    Pen = penalties(go, ge)
    m, mm = match, mismatch
    s3v = [3 * m, m + 2 * mm, 3 * mm] if sop else [3 * m, 2 * (m + mm), 3 * mm]
    s3max, s3min, s2max, s2min = max(s3v), min(s3v), max(m, mm), min(m, mm)
    scmax = [s3max, 0, 0, 0, s2max, s2max, s2max]
    scmin = [s3min, 0, 0, 0, s2min, s2min, s2min]
    dq = [3, 1, 1, 1, 2, 2, 2]
    gain = max(0.0, max((scmax[T] - int(Pen[T][s])) / dq[T] for T in range(7) for s in range(7)))
    hi = int(np.floor(gain * (la + lb + lc) + 1e-9))
    bestlo = min(la, lb, lc) * min(0, s3min)
    drop = max(0, max(int(Pen[T].max()) - scmin[T] for T in range(7)))
    cdrop = max(0, max(int(Pen[T][s]) - scmin[T] for T in range(7) for s in range(7)))
    return min(0, bestlo - drop) - cdrop, max(hi, 0)


def vi_bias(max_la, max_lb, max_lc, match=1, mismatch=-1, go=2, ge=1, sop=False):
    """The bias use_vi (csrc/pencil_kernel.hip) gives the integer-pattern cell,
    or 0 where it keeps the float cell: the proven range rescaled to the triple
    extended to (P, LB + 2 NW, 128 M) by symbols that never match, widened by
    pencil_slack and lam times the extended coordinate sum, times 8, inside
    [0x0400, 0x7BFF]. (Of use_vs' own conditions only lam = GE = -MISMATCH >= 1,
    GO >= GE, 128 < LC <= 256 and the f16 range are repeated here.)"""
    if not (128 < max_lc <= 256) or ge < 1 or ge != -mismatch or go < ge or abs(match - mismatch) > 7:
        return 0
    lo, hi = value_bound(max_la, max_lb, max_lc, match, mismatch, go, ge, sop)
    slack = 8 * max(abs(match), abs(mismatch)) + 4 * max(abs(go), abs(ge))
    q = max_la + max_lb + max_lc
    if lo - slack < -2048 or hi + ge * q + slack > 2048:
        return 0
    P = -(-max(max_la, 256) // 4) * 4
    e = (P, max_lb + 2 * NW, 256)
    mn, e_mn, e_q = min(max_la, max_lb, max_lc), min(e), sum(e)
    lo_e = -((-min(lo, 0) * e_mn + mn - 1) // mn)
    hi_e = ((max(hi, 0) + 1) * e_q + q - 1) // q
    v_lo, v_hi = lo_e - slack, hi_e + ge * e_q + slack
    if 8 * (v_hi - v_lo) > VI_HI - VI_LO:
        return 0
    return VI_LO - 8 * v_lo


# The end search's key (pencil_common.h: end_fold): per position and half
# {score + 2048 : 4095 - (x - 1) : 255 - lap} in 12 + 12 + 8 bits, folded with an
# unsigned max; the wave and z join it in the final reduction (end_key64).
M32 = 0xFFFFFFFF


def end_key64(key, w, k):
    y = (255 - (key & 255)) * NW + w + 1
    return ((key >> 8) << 32) | ((0xFFFF - y) << 16) | (0xFFFF - (k + 1))


def end_decode(key64):
    """(score, (x, y, z)) of a reduced key."""
    top = key64 >> 32
    return (top >> 12) - 2048, (4095 - (top & 4095) + 1, 0xFFFF - ((key64 >> 16) & 0xFFFF), 0xFFFF - (key64 & 0xFFFF))


def end_reduce(keys, lc):
    """keys[w][i, lane, h] -> the workgroup's key: per position slot (the array),
    then per wave, then across the waves, as the kernel reduces them."""
    best = 0
    for w in range(NW):
        wave = 0
        M = keys[w].shape[0]
        for i in range(M):
            for lane in range(64):
                for h in range(2):
                    k, key = 64 * M * h + M * lane + i, int(keys[w][i, lane, h])
                    if k < lc and key:
                        wave = max(wave, end_key64(key, w, k))
        best = max(best, wave)
    return best


def emulate(triples, match=1, mismatch=-1, go=2, ge=1, sop=False, vs=False, shifted=None, garbage_seed=None,
            ring_garbage_seed=None, read_prev=False, int_bits=False, bias=None, events=None, end=None,
            max_lens=None, shared_fetch=False, fetch_shift=0):
    """Scores of one workgroup's unit: one triple, or two (TWO mode: LC <= 64).
    Returns a list of scores (one per triple). `garbage_seed` starts the LDS
    record slots, `ring_garbage_seed` the global ring, with garbage (what an
    earlier launch left in the workspace): a ring row read before this unit
    wrote it then spoils the score.

    end = "face" | "any": the END instantiation's fold (one triple): returns
    [(score, (x1, y1, z1))]; a tuple of modes folds each in the same replay and
    returns one such pair per mode. events["end_cands"], when the caller put a
    list there, receives every folded candidate as (mode, w, i, lane, h, key),
    and events["end_key"][mode] the reduced 64-bit key.

    max_lens = (max_la, max_lb, max_lc): the batch's maxima, from which the
    launch takes its geometry (M, P, the bias) -- a triple of a ragged batch
    is replayed as the kernel runs it, inside a larger cube."""
    two = len(triples) == 2
    end_modes = () if end is None else (end,) if isinstance(end, str) else tuple(end)
    assert all(m in ("face", "any") for m in end_modes) and not (end_modes and two)
    ekeys = {m: [None] * NW for m in end_modes}
    shifted = (vs and not read_prev) if shifted is None else shifted
    assert vs or not shifted
    assert not read_prev or (vs and not shifted)
    la_, lb_, lc_ = ([len(t[k]) for t in triples] for k in range(3))
    max_la, max_lb, max_lc = (max(la_), max(lb_), max(lc_)) if max_lens is None else max_lens
    assert max_la >= max(la_) and max_lb >= max(lb_) and max_lc >= max(lc_)
    M = 1 if max_lc <= 128 else 2
    assert not two or max_lc <= 64
    KS = 64 if two else 128 * M
    P = max(max_la, 64 if two else 128 * M)
    P = -(-P // M) * M
    if M == 2 and not two:  # as the kernel's pencil_geom: P a multiple of 4
        P = -(-P // 4) * 4
    R = P + RING_EXTRA
    lam = ge if vs else 0
    assert not vs or ge == -mismatch
    assert not int_bits or (vs and read_prev and M == 2 and not two)
    if int_bits and bias is None:
        bias = vi_bias(max_la, max_lb, max_lc, match, mismatch, go, ge, sop)
        assert bias, "use_vi's rule refuses this shape and parameter set"
    if events is None:
        events = {}
    events.setdefault("window", 0)
    events.setdefault("carry", 0)
    track = events.get("range")  # only a caller that put a dict there gets the value ranges
    assert track is None or not int_bits
    lens_h = [np.array([len(trip_[k]) for trip_ in (triples if two else triples * 2)])[None, None, :]
              for k in range(3)]  # [1, 1, 2]: the lengths of each half's triple
    enc = (lambda v: (bias + 8 * v) & 0xFFFF) if int_bits else (lambda v: v)  # a V value as the registers hold it
    Pen = penalties(go, ge)
    f_single, f_pair = -int(Pen[1].min()), -int(Pen[4].min())
    dm = match - mismatch
    lanes = np.arange(64)
    shape = (M, 64, 2)
    i_ = np.arange(M)[:, None, None]
    l_ = lanes[None, :, None]
    h_ = np.arange(2)[None, None, :]
    kpos = (l_ + 0 * h_ + 0 * i_) if two else (64 * M * h_ + M * l_ + i_)   # [M, 64, 2]
    tri_of = (h_ + 0 * l_ + 0 * i_) if two else np.zeros(shape, np.int64)
    trip = triples if two else triples * 2

    def code(seq, idx):  # symbol (mod 4) or -1 past the sequence
        seq = np.asarray(seq, np.int64)
        ok = (idx >= 0) & (idx < len(seq))
        return np.where(ok, seq[np.clip(idx, 0, max(len(seq) - 1, 0))] & 3 if len(seq) else -1, -1)

    def per_half(fn):
        out = np.empty(shape, np.int64)
        for h in range(2):
            out[..., h] = fn(trip[h], h)[..., h]
        return out

    ccode = per_half(lambda t, h: code(t[2], kpos))
    # final cells: t_f per triple
    t_fs, w_fs, k_fs = [], [], []
    for (a, b, c) in (triples if two else triples[:1]):
        la, lb, lc = len(a), len(b), len(c)
        t_fs.append(((lb - 1) // NW) * P + (la - 1) + S * ((lb - 1) % NW) + (lc - 1))
        w_fs.append((lb - 1) % NW)
        k_fs.append(lc - 1)
    T = max(t_fs) + 1
    lag = P - S * (NW - 1)
    fin = [None] * len(t_fs)

    def face_rec(tr):  # the y = 0 row as wave 0 meets it at step tr
        if vs:
            return np.array([enc(lam * (tr + 1)), enc(lam * (tr + 2)), enc(lam * (tr + 2)), enc(lam * (tr + 2))])
        return np.array([f_single, f_pair, f_pair, 0])

    # V-space: wave 0 builds the face records of its steps [0, t_sw) from its own
    # H values (the kernel's first-lap role) and reads the ring from step t_sw,
    # a whole group at least PD steps before the last wave's first row; only the
    # rows of steps [t_sw, lag) are filled. The message form fills every row.
    t_sw = (max(lag - PD, 0) & ~3) if vs else 0
    ring = np.zeros((R, 4) + shape, np.int64)     # [R, 4, M, 64, 2]
    if ring_garbage_seed is not None:
        ring = np.random.default_rng(ring_garbage_seed).integers(*((0, 1 << 16) if int_bits else (-3000, 3000)),
                                                                 ring.shape)
    for tr in (range(t_sw + FILL_FROM, lag) if vs else range(lag, lag + R)):
        ring[(tr - lag) % R] = face_rec(tr % R)[:, None, None, None] * np.ones((1,) + shape, np.int64)
    xr = np.zeros((NW, 4, 4) + shape, np.int64)    # [wave][slot][field]
    if garbage_seed is not None:  # LDS starts with whatever the last kernel left
        xr = np.random.default_rng(garbage_seed).integers(*((0, 1 << 16) if int_bits else (-3000, 3000)), xr.shape)
    if shifted:  # wave 0 seeds lane 0's shifted {Iyz, best} of steps -2, -1 (slots 2, 3): the z = 0
        # face wave 1's position 0 takes at its first steps (H_0(0), H_0(1); no record precedes them)
        for slot, v in ((2, lam * 1), (3, lam * 2)):
            xr[0, slot, 2, 0, 0, :] = v
            xr[0, slot, 3, 0, 0, :] = v
    # shared_fetch: wave 0's LDS copy of the ring rows, slot by slot
    assert (not shared_fetch or (vs and read_prev and M == 2 and not two))
    if shared_fetch:  # (the other modes' callers compare the dict they get back)
        events.setdefault("fetch_in_flight", 0)
        events.setdefault("fetch_unread", 0)
    sf_rng = np.random.default_rng(0x5F)
    sf_garbage = lambda: sf_rng.integers(*((0, 1 << 16) if int_bits else (-3000, 3000)), (4,) + shape)
    xr0 = [dict(step=None, flying=False, data=sf_garbage()) for _ in range(PD)]
    sf_queue = {w: [] for w in ((1, 2) if shared_fetch else ())}  # issuer -> its rows in flight, oldest first

    def sf_step(t):  # after every wave's step t: the issues, then the waits (and what lands at the barrier)
        for w, queue in sf_queue.items():
            issuing = t >= t_sw - PD
            if issuing and not t & 1:
                s_row = t + 6 + (w - 1) + 2 * fetch_shift
                slot = xr0[s_row % PD]
                if slot["flying"] or (slot["step"] is not None and slot["step"] >= t_sw and slot["step"] < T
                                      and t // 2 <= slot["step"] // 2):
                    events["fetch_unread"] += 1
                slot.update(step=s_row, flying=True, data=sf_garbage())
                queue.append((s_row, ring[(s_row - lag) % R].copy()))
            if issuing and t & 1:  # the counted wait before this (odd) step's barrier
                while len(queue) > 2:
                    s_row, data = queue.pop(0)
                    if xr0[s_row % PD]["step"] == s_row:  # (not overwritten by a later fetch)
                        xr0[s_row % PD].update(flying=False, data=data)

    def sf_read(t):  # wave 0's record of step t >= t_sw
        slot = xr0[t % PD]
        if slot["flying"] or slot["step"] != t:
            events["fetch_in_flight"] += 1
            return sf_garbage()
        return slot["data"]

    st = []
    for w in range(NW):
        xpos0 = (P - (S * w) % P) % P
        lap0 = 0 if w == 0 else -1
        i_s, i_p, i_m = (bias, bias, bias) if int_bits else (f_single, f_pair, 0)  # (int: in-window patterns)
        d = dict(oIx=np.full(shape, i_s), shIz=np.full(shape, i_s),
                 svIxy=np.full(shape, i_p), svIyz=np.full(shape, i_p),
                 shIxz=[np.full(shape, i_p), np.full(shape, i_p)],
                 svM=[np.full(shape, i_m, np.int64), np.full(shape, i_m, np.int64)],
                 b=np.full(shape, -1), xpos0=xpos0, lap0=lap0)
        if vs:  # H(s) = lam (y + xpos0) at step s, H(-1) := H(0) - lam
            def h_at(s, w=w):
                u = s - S * w
                lp = u // P
                return lam * (lp * NW + w + 1 + (u - lp * P))
            d["H"] = {0: h_at(0), 1: h_at(1), -1: h_at(0) - lam}
            if w == 0:  # position 0's z = 0 faces at steps 0 and 1 ("shifted in" at steps -1, -2)
                d["shIz"][:] = d["svIyz"][:] = enc(d["H"][0])
                d["shIxz"][1][:] = enc(d["H"][1])
                d["svM"][1][:] = enc(d["H"][0])
        st.append(d)

    def shift(v, face):
        # position k <- k-1; lane 0 register 0: low half the face, high half
        # lane 63's low half of register M-1 (TWO: both halves the face)
        out = np.empty_like(v)
        out[1:] = v[:-1]
        out[0, 1:] = v[M - 1, :-1]
        out[0, 0, 0] = face
        out[0, 0, 1] = face if two else v[M - 1, 63, 0]
        return out

    def prev_read(v, face):
        # read_prev: each (lane, register) reads the record of position k-1 by
        # its address -- register i-1 of the lane, or register M-1 of lane-1 (mod
        # 64) -- both halves as they lie there; then lane 0's register 0 takes
        # {face, lane 63's low half} (TWO: the face in both halves)
        out = np.empty_like(v)
        out[1:] = v[:-1]
        out[0] = np.roll(v[M - 1], 1, axis=0)  # lane l <- lane l-1, lane 0 <- lane 63
        lane63_low = out[0, 0, 0]
        out[0, 0, 1] = face if two else lane63_low
        out[0, 0, 0] = face
        return out

    for t in range(T):
        PH = t & 1
        outs = [None] * NW
        for w in range(NW):
            d = st[w]
            if w == 0 and t < t_sw:  # {H(t), H(t + 1) x 3} in every position
                rec = np.array([enc(d["H"][t]), enc(d["H"][t + 1]), enc(d["H"][t + 1]),
                                enc(d["H"][t + 1])])[:, None, None, None] * \
                    np.ones((1,) + shape, np.int64)
            else:
                rec = (sf_read(t) if shared_fetch else ring[(t - lag) % R]) if w == 0 else xr[w - 1, (t - S) & 3]
            u = (t - S * w - kpos) % P
            acode = per_half(lambda tr, h: code(tr[0], u))
            if track is not None:  # the halves that hold a real cell (x <= LA, y <= LB, z <= LC) at this step
                ua = t - S * w - kpos
                real = (ua >= 0) & (u < lens_h[0]) & ((ua // P) * NW + w < lens_h[1]) & (kpos < lens_h[2])

                def note(name, *vals):
                    for v in vals if real.any() else ():  # each [..., M, 64, 2]
                        v = np.asarray(v)[..., real]
                        lo_, hi_ = track.get(name, (int(v.min()), int(v.max())))
                        track[name] = (min(lo_, int(v.min())), max(hi_, int(v.max())))
            else:
                def note(name, *vals):
                    pass
            inIx, inIy, inIz = d["oIx"].copy(), rec[0].copy(), d["shIz"].copy()
            inIxy, inIyz = d["svIxy"].copy(), d["svIyz"].copy()
            inIxz, inM = d["shIxz"][PH].copy(), d["svM"][PH].copy()
            b = d["b"]
            if d["xpos0"] < KS:  # x = 1 at position xpos0: the x = 0 face, the row's B
                inj = kpos == d["xpos0"]
                row = d["lap0"] * NW + w
                bn = per_half(lambda tr, h: code(tr[1], np.full(shape, row)))
                b = np.where(inj, bn, b)
                d["b"] = b
                if vs:
                    inIx[inj] = inIxy[inj] = inIxz[inj] = enc(d["H"][t])
                    inM[inj] = enc(d["H"][t - 1])
                else:
                    inIx[inj], inIxy[inj], inIxz[inj], inM[inj] = f_single, f_pair, f_pair, 0
            eab = (acode >= 0) & (acode == b)
            eac = (acode >= 0) & (acode == ccode)
            ebc = (b >= 0) & (b == ccode)
            if int_bits:
                started = (t - S * w - kpos) >= 0
                mx = np.maximum

                def seen(v):  # a started half outside the window
                    events["window"] += int((started & ((v < VI_LO) | (v > VI_HI))).sum())
                    return v

                def wadd(v, cst):  # one 32-bit add of the packed constant (signed halves cst)
                    cst = np.broadcast_to(np.asarray(cst, np.int64), shape)
                    low = v[..., 0] + cst[..., 0]
                    events["carry"] += int((((low < 0) | (low > 0xFFFF)) & started[..., 1]).sum())
                    word = (v[..., 0] + (v[..., 1] << 16) + cst[..., 0] + cst[..., 1] * 65536) & 0xFFFFFFFF
                    return seen(np.stack([word & 0xFFFF, word >> 16], -1))

                def mad(e_, w_, v):  # v_pk_mad_u16: per half, mod 2^16
                    return seen((e_ * (w_ & 0xFFFF) + v) & 0xFFFF)

                def over(w8, codes):  # 8 w / code per half, 0 for code 0
                    return np.where(codes > 0, w8 // np.maximum(codes, 1), 0)

                ca, cb, cc = (np.where(v >= 0, 1 << np.maximum(v, 0), 0) for v in (acode, b, ccode))
                e_ab, e_ac = ca & cb, ca & cc
                DMB, DMC = over(8 * dm, cb), over(8 * dm, cc)
                d0, d1 = 2 * (match + mismatch) - 3 * mismatch, 3 * match - 2 * (match + mismatch)
                sXY, sXZ = mad(e_ab, DMB, inIxy), mad(e_ac, DMC, inIxz)
                sYZ = wadd(inIyz, 8 * dm * ebc)
                if sop:
                    sM = wadd(mad(e_ab, DMB, mad(e_ac, DMC, inM)), 8 * (3 * mismatch + 3 * lam + dm * ebc))
                else:
                    sM = mad(e_ab, over(8 * (d0 + d1 * ebc), cb), inM)
                sX, sY, sZ = inIx, inIy, inIz
                Gx, Gy, Gz = mx(mx(sY, sZ), sYZ), mx(mx(sX, sZ), sXZ), mx(mx(sX, sY), sXY)
                best = mx(mx(Gx, Gy), mx(sXY, sM))
                b1 = wadd(best, -8 * (go - ge))
                pXY, pYZ, pXZ = mx(Gz, b1), mx(Gx, b1), mx(Gy, b1)
                c8 = -8 * (go + mismatch + lam)
                qXY, qYZ, qXZ = wadd(pXY, c8), wadd(pYZ, c8), wadd(pXZ, c8)
                nIx = mx(wadd(sX, -8 * lam), mx(qXY, qXZ))
                oIy = mx(wadd(sY, -8 * lam), mx(qXY, qYZ))
                oIz = mx(wadd(sZ, -8 * lam), mx(qYZ, qXZ))
                oIxy, oIyz, oIxz = pXY, pYZ, pXZ
            elif vs:
                sXY, sXZ, sYZ = inIxy + dm * eab, inIxz + dm * eac, inIyz + dm * ebc
                if sop:
                    sM = inM + dm * (eab.astype(np.int64) + ebc + eac) + 3 * mismatch + 3 * lam
                else:
                    sM = inM + np.where(eab, np.where(ebc, 3 * match, 2 * (match + mismatch)) - 3 * mismatch,
                                        0) + 3 * mismatch + 3 * lam
                sX, sY, sZ = inIx, inIy, inIz
                mx = np.maximum
                Gx, Gy, Gz = mx(mx(sY, sZ), sYZ), mx(mx(sX, sZ), sXZ), mx(mx(sX, sY), sXY)
                best = mx(mx(Gx, Gy), mx(sXY, sM))
                b1 = best - (go - ge)
                pXY, pYZ, pXZ = mx(Gz, b1), mx(Gx, b1), mx(Gy, b1)
                cP = go + mismatch + lam
                nIx = mx(sX - lam, mx(pXY, pXZ) - cP)
                oIy = mx(sY - lam, mx(pXY, pYZ) - cP)
                oIz = mx(sZ - lam, mx(pYZ, pXZ) - cP)
                oIxy, oIyz, oIxz = pXY, pYZ, pXZ
                note("in", inM, inIx, inIy, inIz, inIxy, inIyz, inIxz)
                note("sum", sXY, sXZ, sYZ, sM)
                note("max", Gx, Gy, Gz, best, b1, pXY, pYZ, pXZ)
                note("out", sX - lam, sY - lam, sZ - lam, mx(pXY, pXZ) - cP, mx(pXY, pYZ) - cP,
                     mx(pYZ, pXZ) - cP, nIx, oIy, oIz)
            else:  # message form, mismatch not folded (integer arithmetic)
                s2 = lambda e: np.where(e, match, mismatch)
                if sop:
                    s3 = s2(eab) + s2(ebc) + s2(eac)
                else:
                    s3 = np.where(eab, np.where(ebc, 3 * match, 2 * (match + mismatch)), 3 * mismatch)
                Sst = np.stack([inM + s3, inIx, inIy, inIz, inIxy + s2(eab), inIyz + s2(ebc),
                                inIxz + s2(eac)])
                msg = [(Sst - Pen[T_][:, None, None, None]).max(0) for T_ in range(7)]
                best, nIx, oIy, oIz, oIxy, oIyz, oIxz = msg
                note("in", inM, inIx, inIy, inIz, inIxy, inIyz, inIxz)
                note("state", Sst)
                note("term", Sst[None] - Pen[:, :, None, None, None])
                note("msg", *msg)
            for end_m in end_modes:  # the two classes' wave-uniform terms (end_class), then the fold (end_fold)
                la1, lb1, lc1 = len(triples[0][0]), len(triples[0][1]), len(triples[0][2])

                def end_class(xq, lap, row):
                    ok = lap >= 0 and row < lb1
                    lim = la1 if ok else 0
                    q = xq + row + 3
                    top = (16384 - bias - 8 * lam * q) if int_bits else (2048 - lam * q)
                    width = (0 if not ok else la1 if row + 1 == lb1 else 1) if end_m == "face" else lim
                    add = ((top << (17 if int_bits else 20)) + ((4095 - xq) << 8) + (255 - lap)) & M32
                    return (xq - lim + 1) & M32, width, lim, add

                cA = end_class(d["xpos0"], d["lap0"], d["lap0"] * NW + w)
                cB = end_class(d["xpos0"] + P, d["lap0"] - 1, (d["lap0"] - 1) * NW + w)
                zface = (kpos == lc1 - 1) if end_m == "face" else np.zeros(shape, bool)
                inA = ((kpos - cA[0]) & M32) < np.where(zface, cA[2], cA[1])
                inB = ((kpos - cB[0]) & M32) < np.where(zface, cB[2], cB[1])
                hv = (np.asarray(best, np.int64) << (17 if int_bits else 20)) & M32
                cand = np.where(inA | inB, (hv + np.where(inA, cA[3], cB[3]) + (kpos << 8)) & M32, 0)
                ekeys[end_m][w] = cand if ekeys[end_m][w] is None else np.maximum(ekeys[end_m][w], cand)
                if events.get("end_cands") is not None:
                    events["end_cands"] += [(end_m, w, int(i), int(l), int(h), int(cand[i, l, h]))
                                            for i, l, h in np.argwhere(inA | inB)]
            for j, (tf, wf, kf) in enumerate(zip(t_fs, w_fs, k_fs)):
                if t == tf and w == wf:
                    pos = np.argwhere((kpos == kf) & (tri_of == j))[0]
                    fin[j] = int(best[tuple(pos)])
            out = np.stack([oIy, oIxy, oIyz, best])
            if w == NW - 1 and t < KS + S * NW:  # not-started positions publish the y = 0 face
                unstarted = kpos > t - S * w
                fr = face_rec(t + lag)
                for f in range(4):
                    out[f][unstarted] = fr[f]
            outs[w] = out
            # advance: position 0 moves on (wrap: a new row), then the z-shifts
            d["oIx"] = nIx
            d["svIxy"] = rec[1]
            if vs:
                d["H"][t + 2] = d["H"][t + 1] + lam
            d["xpos0"] += 1
            if d["xpos0"] == P:
                d["xpos0"] = 0
                d["lap0"] += 1
                if vs:
                    y = d["lap0"] * NW + w + 1
                    d["H"][t], d["H"][t + 1], d["H"][t + 2] = lam * (y - 1), lam * y, lam * (y + 1)
            if vs:
                h1, h2 = enc(d["H"][t + 1]), enc(d["H"][t + 2])
                d["shIxz"][PH] = shift(oIxz, h2)
                d["shIz"] = shift(oIz, h1)
                if shifted:  # the writer shifted the record; its face is h2 (see above)
                    d["svIyz"] = rec[2].copy()
                    d["svM"][PH] = rec[3].copy()
                    outs[w] = np.stack([out[0], out[1], shift(out[2], h2), shift(out[3], h2)])
                elif read_prev:
                    d["svIyz"] = prev_read(rec[2], h1)
                    d["svM"][PH] = prev_read(rec[3], h1)
                else:
                    d["svIyz"] = shift(rec[2], h1)
                    d["svM"][PH] = shift(rec[3], h1)
            else:
                d["shIxz"][PH] = shift(oIxz, f_pair)
                d["shIz"] = shift(oIz, f_single)
                d["svIyz"] = shift(rec[2], f_pair)
                d["svM"][PH] = shift(rec[3], 0)
        for w in range(NW):
            xr[w, t & 3] = outs[w]
        ring[t % R] = outs[NW - 1]
        if shared_fetch:
            sf_step(t)
    if end_modes:
        events["end_key"] = {m: end_reduce(ekeys[m], len(triples[0][2])) for m in end_modes}
        return [end_decode(events["end_key"][m]) for m in end_modes]
    shifts = [lam * (len(a) + len(b) + len(c)) for (a, b, c) in (triples if two else triples[:1])]
    if int_bits:
        fin = [(f - bias) // 8 for f in fin]
    return [f - s for f, s in zip(fin, shifts)]
