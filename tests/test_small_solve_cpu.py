"""CPU: syl_solve4 (csrc/small_solve.hpp), the order 1 / 2 / 4 solve with complete pivoting behind the small
Sylvester systems of sylvester.hip and ordschur.hpp, built for the host (tests/cpp/small_solve_host.cpp) and held
against exact rational arithmetic (``fractions.Fraction``).

Figure of a computed x for K x = b, evaluated in rationals:
    omega = ||K x - b||_inf / (||K||_inf ||x||_inf + ||b||_inf)
Condition: omega <= max(3 x numpy.linalg.solve's omega on the same system, 3 x the largest such omega over the
test's set, u = 2^-53), the project's margin of 3 over LAPACK; u only matters where LAPACK solves a whole set
exactly.

Sets.  ``planted``: N = 1, 2, 4; the entry of largest modulus (10) at every position, so every row and column
exchange of the first step is taken; 20 seeded N(0, 1) fills each.  ``later``: N = 4 with 10 at (0, 0) and the
largest entry of the trailing block (5) at each of its 9 positions (second-step exchanges), and with 10, 5 on the
diagonal and 2.5 at each of the last block's 4 positions (third step); the fills are 0.3 N(0, 1), and the test
checks in rationals that each step's pivot is the planted one.  ``replaced``: dyadic K = P L U Q of rank N - 1
whose elimination is exact in floating point, so the last pivot is exactly 0 and is replaced by smin = 2^-40: the
flag is 1 and x solves, by the same rule, the system with smin added at the entry that complete pivoting leaves
last.  ``kronecker``: the four forms (sa, sb in {1, 2}) the block kernel builds from R's [a b; -c a] and the S
block with eigenvalues -(a -+ i sqrt(b c)) + 1e-10, op(S) = S and S^T, with smin as the kernel sets it."""
import itertools
import os
import shutil
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EPS = float(np.finfo(np.float64).eps)
U = EPS / 2.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("small_solve") / "small_solve_host")
    cmd = [HIPCC, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "pcsc_eigenvalue_solver_project_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "small_solve_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def solve4(exe, systems):
    """[(flag, x)] of the host build on [(K, b, smin)], one process for the whole set"""
    text = []
    for K, b, smin in systems:
        text.append(f"{len(b)} {float(smin)!r}")
        text.append(" ".join(repr(float(v)) for v in np.asarray(K).ravel()))
        text.append(" ".join(repr(float(v)) for v in b))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(systems)
    out = []
    for ln in lines:
        f = ln.split()
        out.append((int(f[0]), np.array([float(v) for v in f[1:]])))
    return out


def frac(M):
    return [[Fr(float(v)) for v in row] for row in np.atleast_2d(M)]


def omega(K, x, b):
    """the figure above, exactly"""
    Kf, xf, bf = frac(K), [Fr(float(v)) for v in x], [Fr(float(v)) for v in b]
    res = max(abs(sum(kr[j] * xf[j] for j in range(len(xf))) - bi) for kr, bi in zip(Kf, bf))
    den = max(sum(abs(v) for v in kr) for kr in Kf) * max(abs(v) for v in xf) + max(abs(v) for v in bf)
    return float(res / den) if den else (0.0 if res == 0 else float("inf"))


def complete_pivoting(K):
    """Exact elimination with complete pivoting, the first largest entry in row-major order as syl_solve4 takes
    it: [(pivot, original row, original column, number of entries sharing the largest modulus)] per step."""
    A = frac(K)
    n = len(A)
    rows, cols = list(range(n)), list(range(n))
    steps = []
    for s in range(n):
        best = max(abs(A[u][v]) for u in range(s, n) for v in range(s, n))
        ties = [(u, v) for u in range(s, n) for v in range(s, n) if abs(A[u][v]) == best]
        pu, pv = ties[0]
        A[s], A[pu] = A[pu], A[s]
        rows[s], rows[pu] = rows[pu], rows[s]
        for row in A:
            row[s], row[pv] = row[pv], row[s]
        cols[s], cols[pv] = cols[pv], cols[s]
        steps.append((A[s][s], rows[s], cols[s], len(ties)))
        if A[s][s] != 0:
            for u in range(s + 1, n):
                f = A[u][s] / A[s][s]
                A[u] = [a - f * c for a, c in zip(A[u], A[s])]
    return steps


def check(exe, systems, want_flag=0, against=None):
    """the condition of the head of this file on a set; ``against``: the matrices omega is taken against (K)"""
    got = solve4(exe, systems)
    ref = against if against is not None else [K for K, _, _ in systems]
    w_np = [omega(Kr, np.linalg.solve(np.atleast_2d(Kr), b), b) for Kr, (_, b, _) in zip(ref, systems)]
    floor = max(3.0 * max(w_np), U)
    worst = 0.0
    for (flag, x), Kr, (_, b, _), wn in zip(got, ref, systems, w_np):
        w = omega(Kr, x, b)
        worst = max(worst, w)
        assert flag == want_flag
        assert np.all(np.isfinite(x))
        assert w <= max(3.0 * wn, floor), f"omega {w / EPS:.3g} eps, numpy {wn / EPS:.3g} eps on\n{Kr}\n{b}"
    print(f"{len(systems)} systems: worst omega {worst / EPS:.3g} eps, numpy's worst {max(w_np) / EPS:.3g} eps")


def test_planted_largest_entry(exe):
    rng = np.random.default_rng(4100)
    systems = []
    for N in (1, 2, 4):
        for pu, pv in itertools.product(range(N), range(N)):
            for _ in range(20):
                K = rng.standard_normal((N, N))
                K[pu, pv] = np.copysign(10.0, K[pu, pv])
                systems.append((K, rng.standard_normal(N), 1e-300))
                assert complete_pivoting(K)[0][1:3] == (pu, pv)
    assert len(systems) == 420
    check(exe, systems)


def test_second_and_third_step_exchanges(exe):
    rng = np.random.default_rng(4200)
    systems = []
    for step, plants in ((1, (10.0,)), (2, (10.0, 5.0))):
        for pu, pv in itertools.product(range(step, 4), range(step, 4)):
            for _ in range(20):
                K = 0.3 * rng.standard_normal((4, 4))
                for k, v in enumerate(plants):
                    K[k, k] = v
                K[pu, pv] = np.copysign(plants[-1] / 2.0, K[pu, pv])
                steps = complete_pivoting(K)
                assert [s[1:3] for s in steps[:step + 1]] == [(k, k) for k in range(step)] + [(pu, pv)]
                systems.append((K, rng.standard_normal(4), 1e-300))
    assert len(systems) == 20 * (9 + 4)
    check(exe, systems)


def _rank_deficient(N, rng):
    """dyadic P L U Q with U's last diagonal entry 0 and diagonal 64, 8, 1 (N = 4) / 4 (N = 2) above it"""
    if N == 2:
        L = np.array([[1.0, 0.0], [rng.choice([-0.5, 0.5]), 1.0]])
        Um = np.array([[4.0, rng.choice([-2.0, -1.0, 1.0, 2.0])], [0.0, 0.0]])
    else:
        L = np.eye(4) + np.tril(rng.choice([-0.5, -0.25, 0.25, 0.5], (4, 4)), -1)
        Um = np.triu(rng.choice([-1.0, -0.5, 0.5, 1.0], (4, 4)), 1)
        Um[2, 3] = rng.choice([-0.5, 0.5])
        Um += np.diag([64.0, 8.0, 1.0, 0.0])
    return (L @ Um)[rng.permutation(N)][:, rng.permutation(N)]


def test_a_zero_pivot_is_replaced_by_smin(exe):
    rng = np.random.default_rng(4300)
    smin = 2.0 ** -40
    systems, nearby = [], []
    for N in (2, 4):
        for _ in range(20):
            K = _rank_deficient(N, rng)
            steps = complete_pivoting(K)
            assert all(s[3] == 1 for s in steps[:-1]), "a tie: the pivot order would depend on the scan"
            assert all(s[0] != 0 for s in steps[:-1]) and steps[-1][0] == 0
            Kn = K.copy()
            Kn[steps[-1][1], steps[-1][2]] += smin     # P (L (U + smin e e^T)) Q = K + smin e_row e_col^T
            assert Fr(float(Kn[steps[-1][1], steps[-1][2]])) == Fr(float(K[steps[-1][1], steps[-1][2]])) + Fr(smin)
            systems.append((K, rng.standard_normal(N), smin))
            nearby.append(Kn)
    check(exe, systems, want_flag=1, against=nearby)
    # smin below every pivot leaves a regular system alone
    K = np.array([[4.0, 2.0], [2.0, 1.5]])
    (flag, x), = solve4(exe, [(K, np.array([1.0, 1.0]), 0.49)])
    assert flag == 0 and np.array_equal(x, [-0.25, 1.0])
    (flag, x), = solve4(exe, [(K, np.array([1.0, 1.0]), 0.51)])   # the second pivot 0.5 is below smin now
    x1 = 0.5 / 0.51
    assert flag == 1 and np.allclose(x, [(1.0 - 2.0 * x1) / 4.0, x1], rtol=2 * EPS, atol=0.0)


def _kron(Rb, Sb, sa, sb, trans):
    """the matrix sylvester.hip's block kernel builds: unknown u = ua + sa ub holds y(ua, ub)"""
    N = sa * sb
    K = np.zeros((N, N))
    for u, v in itertools.product(range(N), range(N)):
        ua, ub, va, vb = u % sa, u // sa, v % sa, v // sa
        if ub == vb:
            K[u, v] += Rb[ua, va]
        if ua == va:
            K[u, v] += Sb[ub, vb] if trans else Sb[vb, ub]
    return K


def test_kronecker_forms_of_a_nearly_common_pair(exe):
    rng = np.random.default_rng(4400)
    systems = []
    for _ in range(20):
        a, b, c = rng.uniform(1.0, 2.0), rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5)
        g = np.sqrt(b * c)
        Rb = np.array([[a, b], [-c, a]])
        Sb = np.array([[-a + 1e-10, 2.0 * g], [-g / 2.0, -a + 1e-10]])
        for sa, sb, trans in itertools.product((1, 2), (1, 2), (False, True)):
            K = _kron(Rb[:sa, :sa], Sb[:sb, :sb], sa, sb, trans)
            smin = max(EPS * max(np.max(np.abs(Rb)), np.max(np.abs(Sb))), 2.0 ** -1022 / EPS)
            systems.append((K, rng.standard_normal(sa * sb), smin))
    check(exe, systems)
