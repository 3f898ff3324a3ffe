#!/usr/bin/env python3
"""Regenerate tests/golden/jordan48.npz (committed; needs mpmath and an x87 long double).

A 48 x 48 long double matrix A = P (D + N) P: D a well-separated diagonal in which one value stands
twice in a row, N strictly upper triangular with N[k, k + 1] = 1 between the two (a 2 x 2 Jordan
block) and small entries elsewhere, P a product of three Householder reflectors, all formed in long
double.  The rounding of A splits the double eigenvalue into a pair ~sqrt(2^-64) apart; the
fixture holds A and the eigenvalues of that rounded A computed in 60-digit arithmetic (mpmath's
Hessenberg + QR), both as (hi, lo) float64 pairs (exact for the 64-bit significand of A; the
eigenvalues rounded to ~106 bits).  The archive is written with fixed zip timestamps, so a rerun
reproduces the committed file bit for bit.
"""
import io
import os
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
N, PAIR = 48, 20          # order; the Jordan block sits at rows PAIR, PAIR + 1
D0 = 0.3125               # the double eigenvalue


def build():
    rng = np.random.default_rng(4848)
    d = np.linspace(-2.0, 2.0, N).astype(LD) + LD(2) ** -60 * rng.uniform(-1, 1, N).astype(LD)
    d[PAIR] = d[PAIR + 1] = LD(D0)
    T = np.triu(0.02 * rng.standard_normal((N, N)), 1).astype(LD)
    T[PAIR, PAIR + 1] = LD(1)
    T[np.arange(N), np.arange(N)] = d
    A = T.copy()
    for _ in range(3):
        v = rng.standard_normal(N).astype(LD)
        v /= np.sqrt(np.sum(v * v))
        P = np.eye(N, dtype=LD) - 2 * np.outer(v, v)
        A = P @ A @ P
    return A


def split(x):
    """long double array -> (hi, lo) float64, exact"""
    hi = x.astype(np.float64)
    lo = (x - hi.astype(LD)).astype(np.float64)
    assert np.all(hi.astype(LD) + lo.astype(LD) == x)
    return hi, lo


def mp_split(z):
    hi = float(z)
    return hi, float(z - mp.mpf(hi))


def main():
    assert np.finfo(LD).nmant == 63, "needs the x87 80-bit long double"
    A = build()
    a_hi, a_lo = split(A)
    mp.mp.dps = 60
    M = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            M[i, j] = mp.mpf(float(a_hi[i, j])) + mp.mpf(float(a_lo[i, j]))
    ev = mp.eig(M, left=False, right=False)
    ev = sorted((mp.mpc(e) for e in ev), key=lambda z: (float(z.real), float(z.imag)))
    out = np.array([mp_split(z.real) + mp_split(z.imag) for z in ev], dtype=np.float64)   # re.hi re.lo im.hi im.lo
    arrays = {"a_hi": a_hi, "a_lo": a_lo, "eig": out, "pair_value": np.array([D0])}
    path = os.path.join(HERE, "jordan48.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0))
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
