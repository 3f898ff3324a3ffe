"""GPU: backward error of to_hessenberg and qr_decompose at the edges of their dispatch, in all four dtypes.

to_hessenberg returns H only.  Reducing the embedding of tests/householder_ref.py makes the device's own panel,
GEMV and rank-k kernels hand back the Q of A = Q H Q^H as well, so H is tied to A by a similarity and not just
compared entry by entry.  Conditions, with "ref" the figure of the reference algorithm (to_hessenberg.hpp:38-77,
qr_decompose.hpp:46-85) run in the same precision on the same matrix:

    r <= max(2, 3 r_ref),   o <= max(2, 3 o_ref),   everything finite,   rest_max == 0

    r = ||Q H Q^H - A||_F / (n eps ||A||_F)        o = ||Q^H Q - I||_F / (n eps)                (Hessenberg)
    r = ||Q R - A||_F / (max(m, n) eps ||A||_F)    o = ||Q^H Q - I||_F / (m eps)                (QR)

(the rule of tests/test_gpu_eigh.py; tests/test_householder_ref_cpu.py shows that the reference alone stays
below 1 and that three planted defects fail it).  Above n = 600 the reference is too slow for a test and
r <= 2, o <= 2 alone apply.

The two orders above n = 260 use the 8-column probe form of hess_figures.  For a fixed error matrix E and a
standard normal X (n x 8), E ||E X||_F^2 = 8 ||E||_F^2 and ||X||_F^2 ~ 8 n, so a probe figure is the full
figure / sqrt(n) in the mean; the squared norm's relative spread over X is at most sqrt(2 / 8) = 0.5, so
sqrt(n) * figure exceeds twice the full figure only beyond 3 sigma.  Those cases therefore also hold
sqrt(n) * figure <= 4, the fixed cap of 2 carried over to the probe form.

Every measured figure is written to profiles/householder_accuracy.json.
"""
import json
import os

import numpy as np
import pytest

import pcsc_eigenvalue_solver_project_amd as E
from oracle import oracle as O

import householder_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_JSON = os.path.join(ROOT, "profiles", "householder_accuracy.json")
_figures = {}
_reference = {}

DT = pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_name)


def _record(key, **kw):
    if not _figures and os.path.exists(ACCURACY_JSON):   # a partial run keeps the other cases' figures
        with open(ACCURACY_JSON) as f:
            _figures.update(json.load(f))
    _figures[key] = {k: (bool(v) if isinstance(v, (bool, np.bool_)) else float(v)) for k, v in kw.items()}
    os.makedirs(os.path.dirname(ACCURACY_JSON), exist_ok=True)
    with open(ACCURACY_JSON, "w") as f:
        json.dump(_figures, f, indent=1, sort_keys=True)
        f.write("\n")


def _forward_tolerance(dtype):
    """The project's existing forward tolerances (test_gpu_qr.py, test_gpu_single.py), relative to ||A||_F."""
    return 2e-5 if R.is_single(dtype) else 1e-12


def _fro(A):
    return float(np.linalg.norm(A.astype(R.double_type(A.dtype))))


def _hess_reference(kind, n, pad, dtype):
    """(r_ref, o_ref, H_ref) of the embedded reference run, computed once per case and left unchanged."""
    key = (kind, n, pad, np.dtype(dtype).name)
    if key not in _reference:
        A = R.matrix(kind, n, dtype, R.seed_of(kind, n))
        M, p = R.embed(A, pad)
        Q, H, rest = R.split(R.reference_hess(M), n, p)
        assert rest == 0
        H = np.array(H)
        H.setflags(write=False)
        _reference[key] = R.hess_figures(A, Q, H) + (H,)
    return _reference[key]


def check_embedded(ctx, tag, kind, n, pad, dtype):
    A = R.matrix(kind, n, dtype, R.seed_of(kind, n))
    M, p = R.embed(A, pad)
    HM = E.to_hessenberg(ctx, M)
    assert HM.dtype == A.dtype and HM.shape == M.shape
    assert np.all(np.isfinite(HM))
    Q, H, rest = R.split(HM, n, p)
    r, o = R.hess_figures(A, Q, H)
    key = f"hessenberg/{tag}/{kind}/n{n}+pad{pad}/{R.dtype_name(dtype)}"
    if n <= R.REFERENCE_LIMIT:
        r_ref, o_ref, H_ref = _hess_reference(kind, n, pad, dtype)
        forward = float(np.abs(R.align_phases(H, H_ref)[0] - H).max()) / _fro(A)
        _record(key, r=r, o=o, r_ref=r_ref, o_ref=o_ref, forward=forward, rest_max=rest)
        print(f"{key}: r={r:.3f} (ref {r_ref:.3f}) o={o:.3f} (ref {o_ref:.3f}) forward={forward:.2e} rest={rest:g}")
    else:
        r_ref = o_ref = 0.0
        _record(key, r=r, o=o, rest_max=rest)
        print(f"{key}: r={r:.4f} o={o:.4f} rest={rest:g}")
    assert rest == 0
    if M.shape[0] >= 64:
        assert np.abs(np.tril(H, -2)).max() == 0
    assert R.within_cap(r, r_ref)
    assert R.within_cap(o, o_ref)
    if n > R.PROBE_ABOVE:
        assert np.sqrt(n) * r <= 4 and np.sqrt(n) * o <= 4
    return H


# ------------------------------------------------------------------ Hessenberg, embedded
# N = 2 n + pad: 40 per-reflector kernels; 63 the last unblocked order; 64 the first blocked one (62 reflector
# columns, partial last panel); 65 (63 columns); 66 (64 columns: whole panels, trailing width 2 after the last);
# 67 a one-reflector last panel; 133 A starts mid-panel (p = 68); 260 A starts at p = 130; 527 the early
# panels' W = V^H A GEMMs reach 512 rows.
@DT
@pytest.mark.parametrize("kind", R.HESS_EMBEDDED_KINDS)
@pytest.mark.parametrize("n,pad", R.HESS_EMBEDDED)
def test_hessenberg_embedded(ctx, n, pad, kind, dtype):
    check_embedded(ctx, "default", kind, n, pad, dtype)


# N = 1200: split-K GEMM (kk >= 512) on live reflectors; N = 2100: the 72-block grid with the two-level barrier
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=R.dtype_name)
@pytest.mark.parametrize("n,pad", R.HESS_EMBEDDED_LARGE)
def test_hessenberg_embedded_large(ctx, n, pad, dtype):
    check_embedded(ctx, "default", "random", n, pad, dtype)


@DT
@pytest.mark.parametrize("kind", R.HESS_EMBEDDED_KINDS)
@pytest.mark.parametrize("n,pad", R.HESS_FALLBACK)
def test_hessenberg_embedded_fallback_panel(ctx, n, pad, kind, dtype, monkeypatch):
    """The one-launch-per-column panel (hess_panel_col, hess_gemv, hess_y): what runs wherever a cooperative
    launch is unavailable, at the first blocked order (N = 64), with a one-reflector last panel (N = 67), with
    A starting mid-panel (N = 133) and at N = 260.  EIGSOL_HESS_NO_COOP is read per call."""
    monkeypatch.setenv("EIGSOL_HESS_NO_COOP", "1")
    check_embedded(ctx, "no_coop", kind, n, pad, dtype)


# ------------------------------------------------------------------ Hessenberg, direct
def _double_reference(A):
    return O.hessenberg(A.astype(R.double_type(A.dtype)))


@DT
@pytest.mark.parametrize("kind", R.HESS_DIRECT_KINDS)
@pytest.mark.parametrize("n", R.HESS_DIRECT)
def test_hessenberg_direct_forward(ctx, n, kind, dtype):
    """H against the fp64 oracle within the project's forward tolerances (1e-12 ||A||_F; 2e-5 ||A||_F after
    align_phases in single precision), and exact zeros where the algorithm leaves them:
    * a skipped reflector leaves its column untouched, so the planted zeros below it come back as exact zeros:
      column 0 of zerotails, every planted block of blocks (the other planted tails of zerotails are filled by
      earlier reflectors before their own is formed; below N = 64 the per-reflector kernels, like the
      reference, then leave rounding residue there);
    * from N = 64 the blocked path writes exact zeros below the subdiagonal."""
    A = R.matrix(kind, n, dtype, R.seed_of(kind, n))
    H = E.to_hessenberg(ctx, A)
    assert H.dtype == A.dtype and np.all(np.isfinite(H))
    H_ref = _double_reference(A)
    if R.is_single(dtype):                 # fp64: no alignment, as test_gpu_qr.py compares
        H_ref = R.align_phases(H, H_ref)[0]
    forward = float(np.abs(H.astype(H_ref.dtype) - H_ref).max()) / _fro(A)
    _record(f"hessenberg/direct/{kind}/n{n}/{R.dtype_name(dtype)}", forward=forward)
    print(f"direct {kind} n={n} {R.dtype_name(dtype)}: forward={forward:.2e}")
    assert forward <= _forward_tolerance(dtype)
    if kind == "zerotails":
        assert np.abs(H[2:, 0]).max() == 0
        if n == 3:
            assert np.array_equal(H, A)
    if kind == "blocks":
        for k in R.skip_columns(n, dtype):
            assert np.abs(H[k + 2:, :k + 2]).max(initial=0) == 0
    if n >= 64:
        assert np.abs(np.tril(H, -2)).max() == 0


@DT
@pytest.mark.parametrize("n", R.HESS_ALREADY)
def test_hessenberg_of_a_hessenberg_matrix_is_itself(ctx, n, dtype):
    A = R.matrix("hess", n, dtype, n)
    assert np.array_equal(E.to_hessenberg(ctx, A), A)


@DT
@pytest.mark.parametrize("sign", [1, -1])
def test_hessenberg_power_of_two_scaling(ctx, sign, dtype):
    """to_hessenberg(s A) against s to_hessenberg(A), s = 2^+-200 (2^+-40 in single precision), N = 66: finite
    and within the forward tolerance scaled by s.  Whether it is bitwise is recorded, not asserted."""
    e = sign * (40 if R.is_single(dtype) else 200)
    A = R.matrix("random", 66, dtype, 66)
    sA = np.ldexp(A.real, e) + (1j * np.ldexp(A.imag, e) if R.is_complex(dtype) else 0)
    sA = np.asfortranarray(sA.astype(dtype))
    assert np.all(np.isfinite(sA)) and np.array_equal(np.ldexp(sA.real, -e), A.real)
    H, Hs = E.to_hessenberg(ctx, A), E.to_hessenberg(ctx, sA)
    assert np.all(np.isfinite(Hs))
    back = np.ldexp(Hs.real, -e) + (1j * np.ldexp(Hs.imag, -e) if R.is_complex(dtype) else 0)
    diff = float(np.abs(back.astype(R.double_type(dtype)) - H.astype(R.double_type(dtype))).max()) / _fro(A)
    bitwise = bool(np.array_equal(back.astype(dtype), H))
    _record(f"hessenberg/scaling/2^{e}/{R.dtype_name(dtype)}", forward=diff, bitwise=bitwise)
    print(f"scaling 2^{e} {R.dtype_name(dtype)}: diff={diff:.2e} bitwise={bitwise}")
    assert diff <= _forward_tolerance(dtype)


# ------------------------------------------------------------------ QR
def _qr_reference(tag, A):
    key = ("qr", tag, A.shape, A.dtype.name)
    if key not in _reference:
        Q, Rr = R.reference_qr(A)
        _reference[key] = R.qr_figures(A, Q, Rr)
    return _reference[key]


def check_qr(ctx, tag, mode, A):
    m, n = A.shape
    Q, Rr = E.qr_decompose(ctx, A)
    assert Q.dtype == A.dtype and Rr.dtype == A.dtype and Q.shape == (m, m) and Rr.shape == (m, n)
    assert np.all(np.isfinite(Q)) and np.all(np.isfinite(Rr))
    r, o = R.qr_figures(A, Q, Rr)
    r_ref, o_ref = _qr_reference(tag, A)
    D = R.double_type(A.dtype)
    Qo, Ro = O.qr_decompose(A.astype(D))
    forward = float(np.abs(Rr.astype(D) - Ro).max()) / _fro(A), float(np.abs(Q.astype(D) - Qo).max())
    key = f"qr/{mode}/{tag}/{m}x{n}/{R.dtype_name(A.dtype)}"
    _record(key, r=r, o=o, r_ref=r_ref, o_ref=o_ref, forward=forward[0], forward_q=forward[1])
    print(f"{key}: r={r:.3f} (ref {r_ref:.3f}) o={o:.3f} (ref {o_ref:.3f}) forward R {forward[0]:.2e} Q {forward[1]:.2e}")
    if min(m, n) >= 64:
        assert np.abs(np.tril(Rr, -1)).max() == 0
    assert R.within_cap(r, r_ref)
    assert R.within_cap(o, o_ref)
    return Q, Rr, forward


# per-reflector kernels below min(m, n) = 64; blocked with one launch per column below m = 256; the cooperative
# panel from m = 256 (255 / 256 / 257 around it, min(m, n) = 64, 96, 256 exact multiples of the panel width,
# real square input whose last column has an empty tail)
@DT
@pytest.mark.parametrize("m,n", R.QR_UNBLOCKED + R.QR_BLOCKED + R.QR_COOP)
def test_qr_backward_error(ctx, m, n, dtype):
    check_qr(ctx, "random", "default", R.rectangle(m, n, dtype, R.seed_of("qr", m, n)))


@DT
@pytest.mark.parametrize("m,n", R.QR_NO_COOP)
def test_qr_backward_error_fallback_panel(ctx, m, n, dtype, monkeypatch):
    """EIGSOL_QR_COOP=0: one qr_panel_col launch per column, what runs wherever a cooperative launch is
    unavailable."""
    monkeypatch.setenv("EIGSOL_QR_COOP", "0")
    check_qr(ctx, "random", "no_coop", R.rectangle(m, n, dtype, R.seed_of("qr", m, n)))


@DT
@pytest.mark.parametrize("n", [40, 130])
def test_qr_of_an_upper_triangular_matrix(ctx, n, dtype):
    """Every tail is zero: every reflector is skipped (qr_decompose.hpp:54-56), Q = I and R = A exactly."""
    A = np.asfortranarray(np.triu(R.rectangle(n, n, dtype, n)))
    Q, Rr = E.qr_decompose(ctx, A)
    assert np.array_equal(Q, np.eye(n, dtype=dtype))
    assert np.array_equal(Rr, A)


@DT
def test_qr_zero_columns_and_zero_pivot(ctx, dtype):
    """130 x 97 with columns 31, 32 and 40 zero (a panel's last and first column and one inside: skipped beside
    live ones, the columns stay exactly zero) and A[0, 0] = 0 over a live tail (sign = 1, qr_decompose.hpp:59-63);
    fp64 / c128 also forward against the oracle within 1e-12, as test_gpu_qr.py compares."""
    A = R.rectangle(130, 97, dtype, 13097)
    A[:, [31, 32, 40]] = 0
    A[0, 0] = 0
    Q, Rr, forward = check_qr(ctx, "zero_columns", "default", A)
    assert np.abs(Rr[:, [31, 32, 40]]).max() == 0
    if not R.is_single(dtype):                 # |R - R_ref| <= 1e-12 ||A||_F and |Q - Q_ref| <= 1e-12 m
        assert forward[0] <= 1e-12 and forward[1] <= 1e-12 * 130


@DT
def test_qr_rank_three(ctx, dtype):
    """130 x 97 of rank 3: from the fourth column on the reflectors are made of rounding residue, so only r and
    o apply, not a forward comparison."""
    rng = np.random.default_rng(3)
    U, V = R.normal(rng, (130, 3), dtype), R.normal(rng, (3, 97), dtype)
    check_qr(ctx, "rank3", "default", np.asfortranarray((U @ V).astype(dtype)))
