"""CPU: the chase schedule of the multishift QR sweeps (csrc/chase_schedule.hpp: ``chase_next_round`` and the two
drivers' (C, nbg) plans), built for the host (tests/cpp/chase_schedule_host.cpp) and run once on every geometry.

Geometries: (a) the drivers' own plans for every active-block order N = 60..1300 with l in {0, 1, 5}, real
(kWin = 96) and complex (kWin = 64); (b) a free grid, nbg = 1..16 and C = 1..8 (real) or nbg = 1..8 and C = 1..4
(complex), N from 3 nbg + 2 to 700 in steps of 7, l = 2.

Conditions: 1. no geometry reports an internal error; 2. each group's rounds tile [0, Tg); 3. within a round
e_q <= s_(q-1); 4. for every step t of a round and every bulge j < nbg with l <= k = l + t - 3 j <= ihi - 1 the
rows max(k - 1, max(0, l - 1)) .. min(k + 3, ihi) lie in [s, e) (a violation would be an LDS access outside the
chase kernel's window); 5. the rounds equal, field for field, those of ``parent_rounds`` below, a transcription
of the loop that francis.hip and zfrancis.hip each carried before the schedule became one function."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def plan_real(N):
    nb = min(32, max(1, N // 8))
    C = max(1, min(8, nb // 4, 1 + N // (4 * (96 + 12))))
    return C, min(nb // C, 16)


def plan_cplx(N):
    nb = min(32, max(1, N // 16))
    C = max(1, min(4, (nb + 7) // 8, 1 + N // (4 * (64 + 12))))
    return C, max(1, min(8, nb // C))


def geometries():
    """(input line, (l, ihi, C, nbg, kWin)) of every case."""
    out = []
    for kind, kwin, plan in (("real", 96, plan_real), ("cplx", 64, plan_cplx)):
        for N in range(60, 1301):
            for l in (0, 1, 5):
                out.append((f"{kind} {N} {l}", (l, l + N - 1) + plan(N) + (kwin,)))
    for kwin, max_nbg, max_c in ((96, 16, 8), (64, 8, 4)):
        for nbg in range(1, max_nbg + 1):
            for C in range(1, max_c + 1):
                for N in range(3 * nbg + 2, 701, 7):
                    out.append((f"free {kwin} {N} 2 {C} {nbg}", (2, N + 1, C, nbg, kwin)))
    return out


@functools.lru_cache(maxsize=None)
def _parent_window(l, ihi, nbg, kWin, tl, Tg):
    """The window of a group at its local step tl and the step at which its round must end."""
    if tl <= 3 * (nbg - 1):
        s = max(0, l - 1)
    else:
        s = max(0, l + tl - 3 * (nbg - 1) - 1)
    e = min(s + kWin, ihi + 1)
    kmax = ihi - 1 if e == ihi + 1 else e - 4
    tl1 = tl
    while tl1 < Tg:
        blead = max(0, int((l + tl1 - (ihi - 1) + 2) / 3))   # C's division truncates
        if blead >= nbg:
            tl1 = Tg
            break
        if l + tl1 - 3 * blead > kmax:
            break
        tl1 += 1
    return s, e, tl1


def parent_rounds(l, ihi, C, nbg, kWin):
    """The drivers' loop before the refactor: (rounds, error); a round is a list of [g, s, e, t0, t1]."""
    G = kWin + 3 * nbg
    Tg = (ihi - 1 - l) + 3 * (nbg - 1) + 1
    T = (C - 1) * G + Tg
    rounds, t0 = [], 0
    while t0 < T:
        t1, wins = T, []
        for g in range(C):
            tl = t0 - g * G
            if tl < 0:
                t1 = min(t1, g * G)
                break
            if tl >= Tg:
                continue
            s, e, tl1 = _parent_window(l, ihi, nbg, kWin, tl, Tg)
            t1 = min(t1, tl1 + g * G)
            wins.append([g, s, e, tl, 0])
        if not wins and t1 > t0:
            t0 = t1
            continue
        if t1 <= t0 or not wins:
            return rounds, "window did not advance"
        for q, w in enumerate(wins):
            w[4] = t1 - w[0] * G
            if q > 0 and w[2] > wins[q - 1][1]:
                return rounds, "windows overlap"
        rounds.append(wins)
        t0 = t1
    return rounds, None


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    """[(geometry, rounds, status)] of the host build, one process call for all geometries."""
    out = str(tmp_path_factory.mktemp("chase_schedule") / "chase_schedule_host")
    cmd = [HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only",
           "-I" + os.path.join(ROOT, "pcsc_eigenvalue_solver_project_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "chase_schedule_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    geos = geometries()
    r = subprocess.run([out], input="".join(g[0] + "\n" for g in geos), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res, rounds, geo = [], None, None
    for line in r.stdout.split("\n"):
        if line.startswith("geo"):
            geo, rounds = tuple(int(x) for x in line.split()[1:]), []
        elif line.startswith("end"):
            res.append((geo, rounds, int(line.split()[1])))
        elif line:
            v = [int(x) for x in line.split()]
            rounds.append([v[i:i + 5] for i in range(0, len(v), 5)])
    assert len(res) == len(geos) == 22962
    assert [g for g, _, _ in res] == [g[1] for g in geos]   # the header's plans are the drivers' plans
    return res


def test_no_internal_error(schedules):
    assert [g for g, _, status in schedules if status != 0] == []


def test_each_groups_rounds_tile_its_steps(schedules):
    for (l, ihi, C, nbg, kWin), rounds, _ in schedules:
        Tg = (ihi - 1 - l) + 3 * (nbg - 1) + 1
        at = [0] * C
        for wins in rounds:
            for g, s, e, t0, t1 in wins:
                assert t0 == at[g] and t1 > t0, (l, ihi, C, nbg, kWin, g, t0, t1)
                at[g] = t1
        assert at == [Tg] * C, (l, ihi, C, nbg, kWin, at)


def test_windows_of_a_round_are_disjoint(schedules):
    for geo, rounds, _ in schedules:
        for wins in rounds:
            assert len({w[0] for w in wins}) == len(wins)
            for q in range(1, len(wins)):
                assert wins[q][2] <= wins[q - 1][1], (geo, wins)
            for g, s, e, t0, t1 in wins:
                assert 0 <= s < e <= geo[1] + 1 and e - s <= geo[4], (geo, wins)


@functools.lru_cache(maxsize=None)
def _rows_touched(l, ihi, nbg):
    """Per group-local step t in [0, Tg): the lowest and the highest row that a live bulge's step touches."""
    Tg = (ihi - 1 - l) + 3 * (nbg - 1) + 1
    k = l + np.arange(Tg)[:, None] - 3 * np.arange(nbg)[None, :]
    live = (k >= l) & (k <= ihi - 1)
    assert live.any(axis=1).all()   # a group has a live bulge at every one of its steps
    lo = np.where(live, np.maximum(k - 1, max(0, l - 1)), ihi + 1).min(axis=1)
    hi = np.where(live, np.minimum(k + 3, ihi), -1).max(axis=1)
    return lo, hi


def test_every_bulge_stays_inside_its_window(schedules):
    for (l, ihi, C, nbg, kWin), rounds, _ in schedules:
        lo, hi = _rows_touched(l, ihi, nbg)
        for wins in rounds:
            for g, s, e, t0, t1 in wins:
                assert lo[t0:t1].min() >= s and hi[t0:t1].max() < e, (l, ihi, C, nbg, kWin, g, s, e, t0, t1)


def test_rounds_equal_the_parents(schedules):
    for geo, rounds, status in schedules:
        want, err = parent_rounds(*geo)
        assert err is None and status == 0 and rounds == want, geo
