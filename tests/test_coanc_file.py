"""instruct_amd/coanc.py: the .coanc file layout the drop-in writes read back, malformed files refused, and chains
combined with their step counts as weights."""
import numpy as np
import pytest

from instruct_amd import coanc


def _sym(n, seed):
    a = np.random.default_rng(seed).random((n, n))
    return (a + a.T) / 2


def _write(path, mean, steps, magic=b"ISGCOANC"):
    """the stated layout in plain numpy: magic, int64 N, int64 steps, the lower triangle row by row"""
    n = mean.shape[0]
    with open(path, "wb") as f:
        f.write(magic)
        f.write(np.array([n, steps], dtype="<i8").tobytes())
        for i in range(n):
            f.write(np.asarray(mean[i, : i + 1], dtype="<f8").tobytes())


@pytest.mark.parametrize("n", [1, 5])
def test_read_round_trips_the_stated_layout(tmp_path, n):
    m = _sym(n, n)
    p = tmp_path / "a.chain1.coanc"
    _write(p, m, 17)
    got, steps = coanc.read(p)
    assert steps == 17 and got.shape == (n, n) and got.dtype == np.float64
    assert np.array_equal(got, m)
    assert p.stat().st_size == 24 + 8 * n * (n + 1) // 2
    q = tmp_path / "b.coanc"
    coanc.write(q, got, steps)
    assert q.read_bytes() == p.read_bytes()


def test_read_takes_the_lower_triangle_row_major(tmp_path):
    """an asymmetric source: only rows i, columns 0 .. i are stored, and they land at [i][j] and [j][i]"""
    m = np.arange(25, dtype=np.float64).reshape(5, 5)
    p = tmp_path / "c.coanc"
    _write(p, m, 3)
    got, _ = coanc.read(p)
    for i in range(5):
        for j in range(i + 1):
            assert got[i, j] == m[i, j] and got[j, i] == m[i, j]


def test_bad_magic_and_short_file_are_rejected(tmp_path):
    m = _sym(5, 2)
    p = tmp_path / "bad.coanc"
    _write(p, m, 4, magic=b"ISGCOANX")
    with pytest.raises(ValueError, match="magic"):
        coanc.read(p)
    _write(p, m, 4)
    raw = p.read_bytes()
    for cut in (raw[:-8], raw[:20], raw[:8], b""):
        p.write_bytes(cut)
        with pytest.raises(ValueError):
            coanc.read(p)
    p.write_bytes(raw + b"\0" * 8)
    with pytest.raises(ValueError):
        coanc.read(p)


def test_combine_weights_by_steps():
    a, b, c = _sym(4, 5), _sym(4, 6), _sym(4, 7)
    mean, steps = coanc.combine([(a, 10), (b, 30), (c, 60)])
    assert steps == 100
    assert np.allclose(mean, 0.1 * a + 0.3 * b + 0.6 * c, rtol=0, atol=4 * 2.0 ** -53)
    same, n = coanc.combine([(a, 7)])
    assert n == 7 and np.array_equal(same, a * 7 / 7)
    # sums that are exact: the combination is the mean over all steps of both chains
    s1, s2 = np.full((2, 2), 3.0), np.full((2, 2), 5.0)
    mean, steps = coanc.combine([(s1 / 4, 4), (s2 / 4, 4)])
    assert steps == 8 and np.array_equal(mean, np.full((2, 2), 1.0))
    with pytest.raises(ValueError):
        coanc.combine([])
    with pytest.raises(ValueError):
        coanc.combine([(a, 1), (_sym(3, 1), 1)])
