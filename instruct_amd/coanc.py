"""Posterior co-ancestry matrices as the drop-in writes them (INSTRUCT_COANC_OUT) and their combination.

File layout, little endian: 8 bytes ``ISGCOANC``, int64 N, int64 steps, then the lower triangle of the mean matrix as N (N + 1) / 2
doubles, row-major (row i holds columns 0 .. i).  The matrix does not depend on how a chain labels its clusters, so the matrices
of several chains of one data set are averaged entry by entry, each weighted by its number of steps.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"ISGCOANC"


def read(path):
    """(mean [N][N] symmetric float64, steps) from a .coanc file"""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 24 or raw[:8] != MAGIC:
        raise ValueError(f"{path}: not a co-ancestry file (magic {raw[:8]!r})")
    n, steps = (int(v) for v in np.frombuffer(raw, dtype="<i8", count=2, offset=8))
    if n < 1 or steps < 1:
        raise ValueError(f"{path}: N {n}, steps {steps}")
    m = n * (n + 1) // 2
    if len(raw) != 24 + 8 * m:
        raise ValueError(f"{path}: {len(raw)} bytes, N {n} needs {24 + 8 * m}")
    mean = np.zeros((n, n), dtype=np.float64)
    mean[np.tril_indices(n)] = np.frombuffer(raw, dtype="<f8", count=m, offset=24)
    mean = mean + np.tril(mean, -1).T
    return mean, steps


def write(path, mean, steps):
    """the same layout from a symmetric matrix (its lower triangle is stored)"""
    mean = np.asarray(mean, dtype=np.float64)
    n = mean.shape[0]
    if mean.shape != (n, n) or n < 1 or steps < 1:
        raise ValueError("write: a square matrix and at least one step")
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(np.array([n, steps], dtype="<i8").tobytes())
        f.write(mean[np.tril_indices(n)].astype("<f8").tobytes())


def combine(chains):
    """step-weighted mean of several chains' (mean, steps): (mean, total steps)"""
    chains = list(chains)
    if not chains:
        raise ValueError("combine: no chains")
    shape = np.asarray(chains[0][0]).shape
    total = 0
    acc = np.zeros(shape, dtype=np.float64)
    for mean, steps in chains:
        mean = np.asarray(mean, dtype=np.float64)
        if mean.shape != shape:
            raise ValueError(f"combine: matrices of {shape} and {mean.shape}")
        if steps < 1:
            raise ValueError("combine: a chain without steps")
        acc += mean * steps
        total += steps
    return acc / total, total
