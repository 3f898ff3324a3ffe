"""CPU: the helpers of tests/householder_ref.py, checked on the oracle alone before any device result is
judged with them.

* The embedding hands back the reference's own H bit for bit, leaves every other block exactly zero, and the
  reference's figures stay inside the cap on their own: r_ref <= 1 and o_ref <= 1 (fp64 / c128, measured at
  most 0.27 and 0.93, both at the smallest orders).
* Single precision, where the reference is the numpy loop in f32 / c64: the same holds (measured at most 0.32
  and 0.95).
* The numpy loop run in fp64 is the oracle's algorithm (agreement to 1e-13 ||A||_F).
* The conditions bite: three small, realistic defects planted in the oracle's own (Q, H) and (Q, R) each fail
  them.
"""
import numpy as np
import pytest

import householder_ref as R
from oracle import oracle as O

DOUBLE = [np.float64, np.complex128]
SINGLE = [np.float32, np.complex64]
CASES = [(kind, n, pad) for kind in R.HESS_EMBEDDED_KINDS for (n, pad) in R.HESS_EMBEDDED]


def _embedded_reference(kind, n, pad, dtype):
    A = R.matrix(kind, n, dtype, R.seed_of(kind, n))
    M, p = R.embed(A, pad)
    Q, H, rest = R.split(R.reference_hess(M), n, p)
    return A, Q, H, rest


@pytest.mark.parametrize("dtype", DOUBLE)
@pytest.mark.parametrize("kind,n,pad", [c for c in CASES if 2 * c[1] + c[2] <= 527])
def test_embedding_returns_the_reference_reduction(kind, n, pad, dtype):
    A, Q, H, rest = _embedded_reference(kind, n, pad, dtype)
    assert H.tobytes() == O.hessenberg(A).tobytes()
    assert rest == 0
    r, o = R.hess_figures(A, Q, H)
    print(f"{kind} ({n},{pad}) {R.dtype_name(dtype)}: r_ref={r:.3f} o_ref={o:.3f}")
    assert r <= 1 and o <= 1


@pytest.mark.parametrize("dtype", SINGLE)
@pytest.mark.parametrize("kind,n,pad", [c for c in CASES if 2 * c[1] + c[2] <= 133])
def test_embedding_single_precision_loop(kind, n, pad, dtype):
    """The numpy loop in f32 / c64: H bitwise the direct run's, zero elsewhere, r_ref <= 1 and o_ref <= 1."""
    A, Q, H, rest = _embedded_reference(kind, n, pad, dtype)
    assert Q.dtype == dtype and H.dtype == dtype
    assert np.array_equal(H, R.hess_loop(A))
    assert rest == 0
    r, o = R.hess_figures(A, Q, H)
    print(f"{kind} ({n},{pad}) {R.dtype_name(dtype)}: r_ref={r:.3f} o_ref={o:.3f}")
    assert r <= 1 and o <= 1


@pytest.mark.parametrize("dtype", DOUBLE)
@pytest.mark.parametrize("kind", ["random", "blocks"])
def test_loop_is_the_oracles_algorithm_in_fp64(kind, dtype):
    A = R.matrix(kind, 40, dtype, 40)
    tol = 1e-13 * np.linalg.norm(A)
    assert np.abs(R.hess_loop(A) - O.hessenberg(A)).max() <= tol
    B = A[:, :27]
    (Q, Rr), (Qo, Ro) = R.qr_loop(B), O.qr_decompose(B)
    assert np.abs(Q - Qo).max() <= tol and np.abs(Rr - Ro).max() <= tol


@pytest.mark.parametrize("dtype", DOUBLE + SINGLE)
def test_families_skip_where_they_say(dtype):
    """blocks: columns k and k + 1 of every planted split are skipped and every other reflector is live, with
    x(0) == 0 at column 7; zerotails: only column 0; hess: all."""
    n = 66
    nb = R.panel_width(dtype)
    live = lambda kind: {k for k, _ in _reflectors(R.matrix(kind, n, dtype, 5))}   # noqa: E731
    skipped = {0, 1, 5, 6, nb - 1, nb, nb + 1, n - 3}
    assert live("blocks") == set(range(n - 2)) - skipped
    assert live("zerotails") == set(range(1, n - 2))
    assert live("hess") == set()
    assert live("random") == set(range(n - 2))
    A = R.matrix("blocks", n, dtype, 5)
    assert A[8, 7] == 0 and np.abs(A[9:nb + 1, 7]).min() > 0
    assert R.hess_loop(A)[8, 7] != 0


def _reflectors(A):
    out = []
    R.hess_loop(A, out)
    return out


def test_align_phases_recovers_a_diagonal_similarity():
    rng = np.random.default_rng(3)
    for dtype in DOUBLE:
        H = np.triu(R.matrix("random", 30, dtype, 9), -1)
        H[12, 11] = 0
        d = np.exp(2j * np.pi * rng.random(30)) if R.is_complex(dtype) else rng.choice([-1.0, 1.0], 30)
        d[0] = 1
        d[12] = d[11]                      # a zero subdiagonal entry keeps d
        G = d[:, None] * H * np.conj(d)[None, :]
        back, dd = R.align_phases(G.astype(dtype), H)
        assert np.abs(dd - d).max() <= 1e-14
        assert np.abs(back - G).max() <= 1e-14 * np.linalg.norm(H)


# ------------------------------------------------------------------ the conditions bite
def _passes(fig, ref):
    return R.within_cap(fig[0], ref[0]) and R.within_cap(fig[1], ref[1])


@pytest.mark.parametrize("dtype", DOUBLE)
def test_hessenberg_conditions_reject_planted_defects(dtype):
    n, pad = 65, 3
    A, Q, H, _ = _embedded_reference("random", n, pad, dtype)
    ref = R.hess_figures(A, Q, H)
    assert _passes(ref, ref)
    eps = np.finfo(dtype).eps
    # one entry of H moved by 4 n eps ||A||_F
    H1 = H.copy()
    H1[10, 20] += 4 * n * eps * np.linalg.norm(A)
    assert not _passes(R.hess_figures(A, Q, H1), ref)
    # the last reflector's right update left out of one row of Q (I - 2 v v^H is its own inverse)
    refl = _reflectors(A)
    k, v = refl[-1]
    assert k == n - 3
    Q2 = Q.copy()
    row = Q2[17, k + 1:]
    Q2[17, k + 1:] = row - 2 * (row @ v) * v.conj()
    assert not _passes(R.hess_figures(A, Q2, H), ref)
    # one reflector applied to Q with the opposite sign of alpha: v' ~ x + alpha e1 instead of x - alpha e1
    Q3 = np.eye(n, dtype=dtype)
    Hk = np.array(A, copy=True)
    for k, v in refl:
        if k == 30:
            x = Hk[k + 1:, k].copy()
            alpha = -(x[0] / abs(x[0])) * np.linalg.norm(x)
            w = x.copy()
            w[0] += alpha
            w /= np.linalg.norm(w)
        else:
            w = v
        Hk[k + 1:, k:] -= 2 * np.outer(v, v.conj() @ Hk[k + 1:, k:])
        Hk[:, k + 1:] -= 2 * np.outer(Hk[:, k + 1:] @ v, v.conj())
        Q3[:, k + 1:] -= 2 * np.outer(Q3[:, k + 1:] @ w, w.conj())
    assert np.abs(Hk - H).max() <= 1e-13 * np.linalg.norm(A)        # the replay itself is the reference's
    assert not _passes(R.hess_figures(A, Q3, H), ref)
    r3, o3 = R.hess_figures(A, Q3, H)
    assert o3 <= 1 and r3 > 2          # still unitary: only the similarity condition sees it


@pytest.mark.parametrize("dtype", DOUBLE)
def test_qr_conditions_reject_planted_defects(dtype):
    m, n = 257, 65
    A = R.rectangle(m, n, dtype, R.seed_of("qr", m, n))
    Q, Rr = R.reference_qr(A)
    ref = R.qr_figures(A, Q, Rr)
    print(f"qr ({m},{n}) {R.dtype_name(dtype)}: r_ref={ref[0]:.3f} o_ref={ref[1]:.3f}")
    assert ref[0] <= 1 and ref[1] <= 1 and _passes(ref, ref)
    eps = np.finfo(dtype).eps
    R1 = Rr.copy()
    R1[10, 20] += 4 * max(m, n) * eps * np.linalg.norm(A)
    assert not _passes(R.qr_figures(A, Q, R1), ref)
    R1 = Rr.copy()
    R1[40, 20] += 4 * max(m, n) * eps * np.linalg.norm(A)       # below the diagonal counts too
    assert not _passes(R.qr_figures(A, Q, R1), ref)
    refl = []
    R.qr_loop(A, refl)
    k, v = refl[-1]
    assert k == n - 1
    Q2 = Q.copy()
    row = Q2[100, k:]
    Q2[100, k:] = row - 2 * (row @ v) * v.conj()
    assert not _passes(R.qr_figures(A, Q2, Rr), ref)
    Q3 = np.eye(m, dtype=dtype)
    Rk = np.array(A, copy=True)
    for k, v in refl:
        w = v
        if k == 30:
            x = Rk[k:, k].copy()
            alpha = -(x[0] / abs(x[0])) * np.linalg.norm(x)
            w = x.copy()
            w[0] += alpha
            w /= np.linalg.norm(w)
        Rk[k:, k:] -= 2 * np.outer(v, v.conj() @ Rk[k:, k:])
        Q3[:, k:] -= 2 * np.outer(Q3[:, k:] @ w, w.conj())
    assert not _passes(R.qr_figures(A, Q3, Rr), ref)


@pytest.mark.parametrize("dtype", SINGLE)
def test_qr_single_precision_loop(dtype):
    """The numpy loop's own QR figures in f32 / c64 (recorded; the device condition is relative to them)."""
    for m, n in [(40, 40), (96, 64), (257, 65)]:
        A = R.rectangle(m, n, dtype, R.seed_of("qr", m, n))
        Q, Rr = R.reference_qr(A)
        assert Q.dtype == dtype and Rr.dtype == dtype
        r, o = R.qr_figures(A, Q, Rr)
        print(f"qr ({m},{n}) {R.dtype_name(dtype)}: r_ref={r:.3f} o_ref={o:.3f}")
        assert r <= 1 and o <= 1
