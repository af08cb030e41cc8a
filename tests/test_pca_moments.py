"""PCA fit from mergeable moments, host side (include/dgn.h: dgn_pca_moments_merge, dgn_pca_solve;
python/dgn/shard.py: allreduce_pca_moments). No GPU: the moments are filled from numpy directly.
Reference and bounds: tests/pca_ref.py."""
import os
import re
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

import dgn
from dgn import abi
import pca_ref as R


@pytest.fixture(scope="module")
def x400():
    return R.pca_input()


def test_tile_constant_mirrors_the_kernel():
    src = open(os.path.join(ROOT, "defect-gnn-cpp_amd", "csrc", "dgn_internal.hpp")).read()
    assert int(re.search(r"kPcaTileRows\s*=\s*(\d+)", src).group(1)) == abi.PCA_TILE_ROWS == dgn.PCA_TILE_ROWS


def test_struct_layout_matches_header():
    import ctypes
    assert ctypes.sizeof(abi.PcaMoments) == 16 + 8 * 35 + 8 * 35 * 35
    m = abi.PcaMoments.from_arrays(3, np.arange(35.0), np.arange(1225.0), skipped=2)
    dgn.lib().dgn_pca_moments_init(ctypes.byref(m))
    assert m.n == 0 and m.skipped == 0 and not m.mean_array().any() and not m.m2_array().any()


@pytest.mark.parametrize("cut", [1, 137, 200, 399])
def test_merge_two_halves_equals_whole(x400, cut):
    a, b = R.moments_of(abi, x400[:cut]), R.moments_of(abi, x400[cut:])
    R.assert_moments(dgn.pca_merge(a, b), x400, f"merge a+b cut {cut}")
    R.assert_moments(dgn.pca_merge(b, a), x400, f"merge b+a cut {cut}")


def test_merge_with_offset_data():
    """Means far from zero (x = 1e6 + normal): every part is centred on its own mean, which is stored
    rounded to f64, so the merge's d = mean_b - mean_a carries up to eta = 4 u max|x| of error per
    column (u |mean| of representation on either side, as much again from an earlier merge's mean
    update) and d d^T na nb / n turns it into a first-order term that a single centring does not have.
    The bound of pca_ref grows by sum over merges of (na nb / n) (|d_a| eta_b + |d_b| eta_a +
    eta_a eta_b); the mean keeps its bound."""
    rng = np.random.default_rng(11)
    x = 1e6 + rng.normal(size=(600, 35))
    spans = ((0, 100), (100, 101), (101, 450), (450, 600))
    m = abi.PcaMoments()
    extra = np.zeros((35, 35), np.longdouble)
    eta = 4 * R.U * np.abs(x).max(axis=0).astype(np.longdouble)
    for lo, hi in spans:
        if lo > 0:
            d = np.abs(x[lo:hi].astype(np.longdouble).mean(0) - x[:lo].astype(np.longdouble).mean(0))
            w = np.longdouble(lo) * (hi - lo) / hi
            extra += w * (np.outer(d, eta) + np.outer(eta, d) + np.outer(eta, eta))
        m = dgn.pca_merge(m, R.moments_of(abi, x[lo:hi]))
    n, mean, m2, mb, sb = R.reference(x)
    assert m.n == n and m.skipped == 0
    assert np.all(np.abs(m.mean_array() - mean) <= mb)
    err = np.abs(m.m2_array() - m2)
    print(f"offset merge: max m2 err / bound = {float(np.max(err / (sb + extra))):.3g}")
    assert np.all(err <= sb + extra)


def test_merge_with_empty_side_is_identity(x400):
    whole, empty = R.moments_of(abi, x400), abi.PcaMoments()
    for m in (dgn.pca_merge(whole, empty), dgn.pca_merge(empty, whole)):
        assert m.n == whole.n
        assert m.mean_array().tobytes() == whole.mean_array().tobytes()
        assert m.m2_array().tobytes() == whole.m2_array().tobytes()
    both = dgn.pca_merge(empty, empty)
    assert both.n == 0 and both.tobytes() == empty.tobytes()


def test_merge_adds_skipped_counts(x400):
    y = x400.copy()
    y[5, 3] = np.nan
    y[300, 0] = np.inf
    m = dgn.pca_merge(R.moments_of(abi, y[:200]), R.moments_of(abi, y[200:]))
    assert m.skipped == 2
    R.assert_moments(m, y, "merge with skipped rows")


def test_solve_matches_numpy(x400):
    mean, comp, ratio = dgn.pca_solve(R.moments_of(abi, x400), 6)
    assert comp.shape == (35, 6) and ratio.shape == (6,)
    R.assert_model_matches_svd(x400, mean, comp, ratio)
    R.assert_model_gap_free(x400, mean, comp, ratio)


def test_solve_k0_and_k35(x400):
    m = R.moments_of(abi, x400)
    mean, comp, ratio = dgn.pca_solve(m, 0)
    assert comp.shape == (35, 0) and ratio.shape == (0,)
    np.testing.assert_allclose(mean, x400.mean(0), rtol=1e-12)
    mean, comp, ratio = dgn.pca_solve(m, 35)
    R.assert_model_matches_svd(x400, mean, comp[:, :6], ratio[:6])
    R.assert_model_gap_free(x400, mean, comp, ratio)
    assert abs(ratio.sum() - 1.0) <= 1e-12 and np.all(np.diff(ratio) <= 0)


def test_sign_rule_holds_for_every_component(x400):
    _, comp, _ = dgn.pca_solve(R.moments_of(abi, x400), 35)
    for c in range(35):
        assert comp[np.argmax(np.abs(comp[:, c])), c] > 0, c


@pytest.mark.parametrize("rows,k", [(400, 36), (400, -1), (1, 6), (0, 6)])
def test_solve_rejects_bad_arguments(x400, rows, k):
    with pytest.raises(dgn.DgnError) as e:
        dgn.pca_solve(R.moments_of(abi, x400[:rows]), k)
    assert e.value.status == 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dgn.shard import allreduce_pca_moments, shard_bounds
    x = R.pca_input()
    lo, hi = shard_bounds(x.shape[0] - 37, world, rank)  # uneven shares: 182 and 181 + 37 rows
    if rank == world - 1:
        hi = x.shape[0]
    merged = allreduce_pca_moments(R.moments_of(abi, x[lo:hi]))
    with open(os.path.join(out_dir, f"m{rank}.bin"), "wb") as f:
        f.write(merged.tobytes())
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_pca_moments_gloo_world2(tmp_path, x400):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    raw = [open(tmp_path / f"m{r}.bin", "rb").read() for r in range(world)]
    assert raw[0] == raw[1]
    R.assert_moments(abi.PcaMoments.from_buffer_copy(raw[0]), x400, "allreduce")
