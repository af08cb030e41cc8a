"""Reference and a-priori error bounds for the PCA moments (shared by test_pca_moments.py and
test_gpu_pca.py; not a test module).

Reference: numpy in longdouble over the finite rows, m = x.mean(0), xc = x - m, M = xc^T xc.
Bounds (u = 2^-53; any correct summation order of n rows stays inside them):
  |d mean_a|  <= 2 n u max_i |x_ia|
  |d m2_ab|   <= 2 n u sum_i |xc_ia| |xc_ib|  +  2 n delta_a delta_b,   delta_a = n u max_i |x_ia|
the first term the rounding of the summation, the second the rounding of the mean (the cross terms of
a mean error e vanish because the centred columns sum to zero, leaving n e_a e_b).
"""
import numpy as np

U = 2.0 ** -53
D = 35


def finite_rows(x):
    x = np.asarray(x, np.float64)
    return x[np.isfinite(x).all(axis=1)]


def reference(x):
    """(n, mean, m2, mean bound, m2 bound) over the finite rows of x, in longdouble."""
    xf = finite_rows(x).astype(np.longdouble)
    n = xf.shape[0]
    if n == 0:
        z = np.zeros(D, np.longdouble)
        return 0, z, np.zeros((D, D), np.longdouble), z, np.zeros((D, D), np.longdouble)
    mean = xf.mean(axis=0)
    xc = xf - mean
    m2 = xc.T @ xc
    amax = np.abs(xf).max(axis=0)
    mean_bound = 2 * n * U * amax
    delta = n * U * amax
    m2_bound = 2 * n * U * (np.abs(xc).T @ np.abs(xc)) + 2 * n * np.outer(delta, delta)
    return n, mean, m2, mean_bound, m2_bound


def _worst(err, bound):
    """Largest err / bound (0 / 0 counts as 0): the figure the tests print before asserting."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.asarray(err / bound, np.float64))
    return float(np.max(r))


def assert_moments(m, x, what=""):
    """The moments struct `m` equals the reference over the finite rows of x within the bounds, counts
    exactly, and its m2 is exactly symmetric."""
    x = np.asarray(x, np.float64)
    n, mean, m2, mb, sb = reference(x)
    assert m.n == n, f"{what}: n {m.n} != {n}"
    assert m.skipped == x.shape[0] - n, f"{what}: skipped {m.skipped} != {x.shape[0] - n}"
    if n == 0:
        return
    gm, g2 = m.mean_array().astype(np.longdouble), m.m2_array().astype(np.longdouble)
    em, e2 = np.abs(gm - mean), np.abs(g2 - m2)
    print(f"{what}: n={n} max mean err/bound={_worst(em, mb):.3g} max m2 err/bound={_worst(e2, sb):.3g}")
    assert np.all(em <= mb), f"{what}: mean off by up to {np.max(em - mb)} beyond the bound"
    assert np.all(e2 <= sb), f"{what}: m2 off by up to {np.max(e2 - sb)} beyond the bound"
    assert np.array_equal(m.m2_array(), m.m2_array().T), f"{what}: m2 not symmetric"


def moments_of(abi, x):
    """PcaMoments filled from numpy directly (longdouble, rounded to f64): no GPU."""
    n, mean, m2, _, _ = reference(x)
    return abi.PcaMoments.from_arrays(n, mean.astype(np.float64), m2.astype(np.float64),
                                      skipped=np.asarray(x).shape[0] - n)


def pca_input(seed=7):
    """The input construction of tests/test_facade.py::test_pca_matches_numpy."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(400, 35)) @ rng.normal(size=(35, 35)) + rng.normal(size=35)


def assert_model_matches_svd(x, mean, comp, ratio):
    """The project's PCA tolerances against numpy's SVD (spectrum under the test's control)."""
    k = comp.shape[1]
    mu = x.mean(0)
    np.testing.assert_allclose(mean, mu, rtol=1e-12)
    _, s, vt = np.linalg.svd(x - mu, full_matrices=False)
    var = s ** 2 / (x.shape[0] - 1)
    np.testing.assert_allclose(ratio, var[:k] / var.sum(), rtol=1e-9)
    for c in range(k):
        v = vt[c] * np.sign(vt[c][np.argmax(np.abs(vt[c]))])
        np.testing.assert_allclose(comp[:, c], v, atol=1e-9)


def assert_model_gap_free(rows, mean, comp, ratio):
    """A model check that does not depend on eigenvalue gaps: orthonormal components, each an
    eigenvector of the covariance numpy computes from the same rows, and the ratios of the covariance's
    own leading eigenvalues."""
    f = finite_rows(rows)
    k = comp.shape[1]
    np.testing.assert_allclose(mean, f.mean(0), rtol=1e-12, atol=1e-300)
    cov = np.cov(f.T)
    assert np.max(np.abs(comp.T @ comp - np.eye(k))) <= 1e-12
    norm = np.linalg.norm(cov, 2)
    lam = np.linalg.eigvalsh(cov)[::-1]
    for c in range(k):
        v = comp[:, c]
        res = np.linalg.norm(cov @ v - ratio[c] * np.maximum(lam, 0).sum() * v)  # lambda_c = ratio_c * sum
        assert res <= 1e-10 * norm, f"component {c}: residual {res} > 1e-10 * {norm}"
        assert v[np.argmax(np.abs(v))] > 0
    np.testing.assert_allclose(ratio, np.maximum(lam[:k], 0) / np.maximum(lam, 0).sum(), rtol=1e-9)
