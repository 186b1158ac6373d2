"""The V-space cell on integer bit patterns (cell_messages_vi in
csrc/pencil_common.h), replayed on packed 32-bit words against the oracle,
cell by cell.

A half holds u = bias + 8 V, V the V-space value of tests/test_cell_algebra.py.
A register pairs two cells that share nothing, as the helix's halves do
(positions k and k + 128): here the low half is cell (x, y, z) of one triple and
the high half the same cell of another, over the larger of the two cubes; a
half past its own triple's lengths is a padding cell (symbol code 0, which
matches nothing), as beside a live cell in the kernel. Per register the replay does
what the kernel does: the match bonuses per half mod 2^16 (v_pk_mad_u16 on the
one-hot code a & b and the weight 8 w / code), the constant adds and subtracts
as ONE 32-bit add of the packed constant, every max on the halves as unsigned
16-bit integers. For every real cell, best decoded as (u - bias) / 8 -
lam (x + y + z) must be the oracle's score of the three prefixes. Two counters
must stay at zero: a half outside [0x0400, 0x7BFF], and a 32-bit add whose low
half carried or borrowed. A bias placed too low must make both fire.

Parameter sets: those of tests/test_cell_algebra.py that the host rule admits
(tools/pencil_emu.py vi_bias, the rule of use_vi) at a shape that pads like
these triples, (12, 12, 140): the RTL constants in both s3 modes and lam = 2.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pencil_emu  # noqa: E402

LO, HI = pencil_emu.VI_LO, pencil_emu.VI_HI
SETS = [{}, dict(match=2, mismatch=-2, GO=3, GE=2), dict(match=1, mismatch=-3, GO=4, GE=1),
        dict(match=3, mismatch=0, GO=2, GE=2), dict(sop=True)]


def _bias(kw):
    return pencil_emu.vi_bias(12, 12, 140, kw.get("match", 1), kw.get("mismatch", -1), kw.get("GO", 2),
                              kw.get("GE", 1), bool(kw.get("sop")))


ADMITTED = [kw for kw in SETS if _bias(kw)]


def vi_cells(t_lo, t_hi, bias, ev, match=1, mismatch=-1, GO=2, GE=1, sop=False):
    """[{(x, y, z): best pattern} of every real cell] of the two triples (low
    halves, high halves); ev counts the two events."""
    lam, dm = GE, match - mismatch
    assert GE == -mismatch
    T = (t_lo, t_hi)
    la, lb, lc = (max(len(t[j]) for t in T) for j in range(3))
    d0, d1 = 2 * (match + mismatch) - 3 * mismatch, 3 * match - 2 * (match + mismatch)
    code = lambda seq, i: (1 << (int(seq[i - 1]) & 3)) if 1 <= i <= len(seq) else 0
    tabs = [{k: {} for k in ("Ix", "Iy", "Iz", "Ixy", "Iyz", "Ixz", "B")} for _ in T]

    def get(k, i, x, y, z):
        if x == 0 or y == 0 or z == 0:
            q = lam * (x + y + z)
            return (bias + 8 * (q - lam if k in ("Ix", "Iy", "Iz") else q)) & 0xFFFF
        return tabs[i][k][(x, y, z)]

    def seen(w):
        for v in (w & 0xFFFF, w >> 16):
            ev["window"] += not LO <= v <= HI
        return w

    def wadd(w, c_lo, c_hi):  # one 32-bit add of c_hi * 65536 + c_lo (signed halves)
        ev["carry"] += not 0 <= (w & 0xFFFF) + c_lo <= 0xFFFF
        return seen((w + c_hi * 65536 + c_lo) & 0xFFFFFFFF)

    def mad(e, wt, v):  # per half, mod 2^16
        return seen(sum((((e >> s & 0xFFFF) * (wt >> s & 0xFFFF) + (v >> s & 0xFFFF)) & 0xFFFF) << s for s in (0, 16)))

    def mx(*ws):  # per half, unsigned
        return max(w & 0xFFFF for w in ws) | max(w >> 16 for w in ws) << 16

    def over(w8, c):  # (8 w / code) mod 2^16, 0 for code 0
        return (w8 // c) & 0xFFFF if c else 0

    pack = lambda f: f(0) | f(1) << 16
    for x in range(1, la + 1):
        a = pack(lambda i: code(T[i][0], x))
        for y in range(1, lb + 1):
            bs = [code(t[1], y) for t in T]
            b = bs[0] | bs[1] << 16
            for z in range(1, lc + 1):
                cs = [code(t[2], z) for t in T]
                c = cs[0] | cs[1] << 16
                ebc = [int(bs[i] != 0 and bs[i] == cs[i]) for i in (0, 1)]
                X = pack(lambda i: get("Ix", i, x - 1, y, z))
                Y = pack(lambda i: get("Iy", i, x, y - 1, z))
                Z = pack(lambda i: get("Iz", i, x, y, z - 1))
                XY = pack(lambda i: get("Ixy", i, x - 1, y - 1, z))
                YZ = pack(lambda i: get("Iyz", i, x, y - 1, z - 1))
                XZ = pack(lambda i: get("Ixz", i, x - 1, y, z - 1))
                Mi = pack(lambda i: get("B", i, x - 1, y - 1, z - 1))
                eab, eac = a & b, a & c
                DMB = pack(lambda i: over(8 * dm, bs[i]))
                DMC = pack(lambda i: over(8 * dm, cs[i]))
                sXY, sXZ = mad(eab, DMB, XY), mad(eac, DMC, XZ)
                sYZ = wadd(YZ, 8 * dm * ebc[0], 8 * dm * ebc[1])
                if sop:
                    k = [8 * (3 * mismatch + 3 * lam + dm * e) for e in ebc]
                    sM = wadd(mad(eab, DMB, mad(eac, DMC, Mi)), k[0], k[1])
                else:
                    sM = mad(eab, pack(lambda i: over(8 * (d0 + d1 * ebc[i]), bs[i])), Mi)
                Gx, Gy, Gz = mx(Y, Z, sYZ), mx(X, Z, sXZ), mx(X, Y, sXY)
                best = mx(Gx, Gy, mx(sXY, sM))
                b1 = wadd(best, -8 * (GO - GE), -8 * (GO - GE))
                pXY, pYZ, pXZ = mx(Gz, b1), mx(Gx, b1), mx(Gy, b1)
                cP = -8 * (GO + mismatch + lam)
                qXY, qYZ, qXZ = wadd(pXY, cP, cP), wadd(pYZ, cP, cP), wadd(pXZ, cP, cP)
                out = dict(Ixy=pXY, Iyz=pYZ, Ixz=pXZ, B=best,
                           Ix=mx(wadd(X, -8 * lam, -8 * lam), qXY, qXZ),
                           Iy=mx(wadd(Y, -8 * lam, -8 * lam), qXY, qYZ),
                           Iz=mx(wadd(Z, -8 * lam, -8 * lam), qYZ, qXZ))
                for k_, w in out.items():
                    tabs[0][k_][(x, y, z)] = w & 0xFFFF
                    tabs[1][k_][(x, y, z)] = w >> 16
    return [{k: v for k, v in tabs[i]["B"].items() if all(k[j] <= len(T[i][j]) for j in range(3))} for i in (0, 1)]


def _oracle_params(orc, kw):
    return orc.default_params(score_bits=0, match=kw.get("match", 1), mismatch=kw.get("mismatch", -1),
                              gap_open=kw.get("GO", 2), gap_extend=kw.get("GE", 1), s3_mode=1 if kw.get("sop") else 0)


def test_admitted_sets():
    assert ADMITTED == [{}, dict(match=2, mismatch=-2, GO=3, GE=2), dict(sop=True)]


@pytest.mark.parametrize("kw", ADMITTED, ids=str)
def test_int_cell_matches_oracle_cell_by_cell(orc, kw):
    rng = np.random.default_rng(9)
    p, bias, lam = _oracle_params(orc, kw), _bias(kw), kw.get("GE", 1)
    triples = [tuple(rng.integers(0, 5, int(rng.integers(1, 13))).astype(np.uint8) for _ in range(3))
               for _ in range(4)]
    triples.append(tuple(np.full(n, 1, np.uint8) for n in (12, 11, 12)))       # all-match: the top of the range
    triples.append(tuple(np.full(n, v, np.uint8) for n, v in ((12, 0), (12, 1), (11, 2))))  # all-distinct: the bottom
    # low half / high half: random beside random, the extremes beside a short random one and beside each other
    for t_lo, t_hi in [(0, 1), (2, 3), (4, 0), (1, 5), (5, 4)]:
        T = (triples[t_lo], triples[t_hi])
        ev = {"window": 0, "carry": 0}
        bests = vi_cells(T[0], T[1], bias, ev, **kw)
        assert ev == {"window": 0, "carry": 0}, (kw, ev)
        for (A, B, C), best in zip(T, bests):
            assert len(best) == len(A) * len(B) * len(C)
            for (x, y, z), u in best.items():
                assert (u - bias) % 8 == 0
                assert (u - bias) // 8 - lam * (x + y + z) == orc.score(A[:x], B[:y], C[:z], p), (kw, x, y, z)


def test_low_bias_is_caught():
    """With the bias too low (-64: V = 8 is the pattern 0, and these cells' V
    run from 0 to about 19) halves leave the window and low halves borrow from
    the high ones."""
    t = ([0] * 6, [1] * 6, [2] * 7)
    ev = {"window": 0, "carry": 0}
    vi_cells(t, t, -64, ev)
    assert ev["window"] > 0 and ev["carry"] > 0, ev
