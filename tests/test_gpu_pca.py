"""PCA moments on the GPU (dgn_dev_pca_accumulate / dgn_host_pca_accumulate, csrc/pca_kernels.hip)
through the C ABI: count, mean and centred scatter of a [rows][35] f64 block in HBM against numpy in
longdouble within the a-priori rounding bounds of tests/pca_ref.py; the non-finite-row rule; bit-exact
repeatability; streaming and host staging; the end-to-end path dev_betti -> pca fit ->
dev_node_features on the POSCAR fixtures; the facade's fit_device and preprocess_betti --stream-pca."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import dgn
from dgn import abi
import pca_ref as R

pytestmark = pytest.mark.gpu

T = abi.PCA_TILE_ROWS
BIN = os.path.join(ROOT, "defect-gnn-cpp_amd", "bin")
POSCARS = os.path.join(GOLDEN, "poscar")
NAMES = ["1", "1046", "1046_1", "1046_2", "1_1", "1_2", "741", "741_1", "741_2"]


@pytest.fixture(scope="module")
def big():
    """3T + 7 random rows with columns of mixed scale and offset; every row-count case is a prefix."""
    rng = np.random.default_rng(5)
    return rng.normal(size=(3 * T + 7, 35)) * (1.0 + np.arange(35) % 5) + rng.normal(size=35)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7])
def test_row_counts_match_reference(ctx, big, rows):
    x = big[:rows]
    R.assert_moments(ctx.dev_pca_accumulate(_dev(x)), x, f"rows {rows}")


def test_zero_rows_leave_moments_untouched(ctx, big):
    m = ctx.dev_pca_accumulate(_dev(big[:70]))
    before = m.tobytes()
    ctx.dev_pca_accumulate(_dev(big[:0]), m)
    assert m.tobytes() == before
    fresh = ctx.dev_pca_accumulate(_dev(big[:0]))
    assert fresh.tobytes() == abi.PcaMoments().tobytes()


def test_bad_arguments_are_rejected(ctx, big):
    import ctypes
    m = abi.PcaMoments()
    lib = dgn.lib()
    d = _dev(big[:4])
    assert lib.dgn_dev_pca_accumulate(ctx.h, d.data_ptr(), -1, ctypes.byref(m)) == 1
    assert lib.dgn_dev_pca_accumulate(ctx.h, None, 4, ctypes.byref(m)) == 1
    assert lib.dgn_dev_pca_accumulate(ctx.h, d.data_ptr(), 4, None) == 1
    assert lib.dgn_host_pca_accumulate(ctx.h, None, 4, ctypes.byref(m)) == 1
    assert m.tobytes() == abi.PcaMoments().tobytes()


def test_offset_data_needs_the_centred_pass(ctx):
    """x = 1e6 + normal(0, 1): the bound is about 1e-12 of the scatter; sum x x^T - n mean mean^T in
    one pass loses about 1e12 * 2^-53 * n of it."""
    rng = np.random.default_rng(9)
    x = 1e6 + rng.normal(size=(4099, 35))
    R.assert_moments(ctx.dev_pca_accumulate(_dev(x)), x, "offset 4099")


def _poisoned(big):
    x = big.copy()
    bad = {0: (3, np.nan), T - 1: (0, np.inf), T: (34, -np.inf), 2 * T - 1: (17, np.nan), x.shape[0] - 1: (5, np.inf)}
    for r, (c, v) in bad.items():
        x[r, c] = v
    x[2 * T:3 * T, 11] = np.nan  # a whole tile of skipped rows
    x[70, :] = np.nan
    return x, len(bad) + T + 1


def test_non_finite_rows_are_left_out(ctx, big):
    x, nbad = _poisoned(big)
    m = ctx.dev_pca_accumulate(_dev(x))
    assert m.skipped == nbad and m.n == x.shape[0] - nbad
    R.assert_moments(m, x, "non-finite rows")


def test_all_rows_skipped_leaves_n_unchanged(ctx, big):
    m = ctx.dev_pca_accumulate(_dev(big[:100]))
    before = m.copy()
    y = big[:T + 3].copy()
    y[:, 7] = np.nan
    ctx.dev_pca_accumulate(_dev(y), m)
    assert m.n == before.n and m.skipped == T + 3
    assert m.mean_array().tobytes() == before.mean_array().tobytes()
    assert m.m2_array().tobytes() == before.m2_array().tobytes()
    only = ctx.dev_pca_accumulate(_dev(y))
    assert only.n == 0 and only.skipped == T + 3 and not only.m2_array().any()


def test_two_calls_are_bit_identical(ctx, big):
    x, _ = _poisoned(big)
    d = _dev(x)
    assert ctx.dev_pca_accumulate(d).tobytes() == ctx.dev_pca_accumulate(d).tobytes()


def test_streaming_three_ragged_chunks(ctx, big):
    m = abi.PcaMoments()
    for lo, hi in ((0, 777), (777, 2 * T + 1), (2 * T + 1, big.shape[0])):
        assert ctx.dev_pca_accumulate(_dev(big[lo:hi]), m) is m
    R.assert_moments(m, big, "three ragged chunks")


def test_host_accumulate_chunk_loop(ctx, big):
    x = big[:1000].copy()
    x[250, 2] = np.nan
    ctx.set_debug(abi.DEBUG_PCA_CHUNK, 100)
    try:
        ctx.host_syncs()
        m = ctx.host_pca_accumulate(x)
        assert ctx.host_syncs() == 10  # one wait per chunk
    finally:
        ctx.set_debug(abi.DEBUG_PCA_CHUNK, 0)
    R.assert_moments(m, x, "host, chunks of 100")
    one = ctx.host_pca_accumulate(x)
    R.assert_moments(one, x, "host, one chunk")
    assert one.tobytes() == ctx.dev_pca_accumulate(_dev(x)).tobytes()


def test_one_host_sync_per_call(ctx, big):
    d = _dev(big)
    ctx.synchronize()
    ctx.host_syncs()
    ctx.dev_pca_accumulate(d)
    assert ctx.host_syncs() == 1


def test_kernel_timing_accounts_bytes_and_flops(ctx, big):
    d = _dev(big)
    ctx.enable_timing(True)
    ctx.reset_timing()
    try:
        ctx.dev_pca_accumulate(d)
        kt = ctx.kernel_times()
    finally:
        ctx.enable_timing(False)
    rows, tiles = big.shape[0], 4
    assert kt["pca_sums"]["bytes"] == rows * 280 + tiles * 2 * 8 * 36
    assert kt["pca_scatter"]["bytes"] == rows * 280 + tiles * 2 * 8 * 630
    assert kt["pca_scatter"]["flops"] >= rows * 2 * 630 and kt["pca_sums"]["launches"] == 1


def _poscar_batch():
    fx = np.load(os.path.join(GOLDEN, "poscar_rc5.npz"))
    pos = [fx[f"{n}/positions"] for n in NAMES]
    return {"lattice": np.stack([fx[f"{n}/lattice"] for n in NAMES]), "positions": np.concatenate(pos),
            "species": np.concatenate([fx[f"{n}/species"] for n in NAMES]).astype(np.int32),
            "atom_offset": np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)}


def test_end_to_end_betti_fit_node_features(ctx):
    import torch
    host = _poscar_batch()
    dev = torch.device("cuda", 0)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    A = host["positions"].shape[0]
    feat = torch.empty((A, 35), dtype=torch.float64, device=dev)
    ctx.dev_betti(batch, 5.0, feat)
    m = ctx.dev_pca_accumulate(feat)
    f = feat.cpu().numpy()
    R.assert_moments(m, f, "POSCAR Betti block")
    assert m.skipped == 0
    mean, comp, ratio = dgn.pca_solve(m, 6)
    R.assert_model_gap_free(f, mean, comp, ratio)
    S, D = int(host["species"].max()) + 1, 4
    embed = np.random.default_rng(3).normal(size=(S, D))
    out = torch.empty((A, D + 6), dtype=torch.float64, device=dev)
    ctx.dev_node_features(batch, _dev(embed), feat, _dev(mean), _dev(comp), out)
    ctx.synchronize()
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :D], embed[host["species"]])
    ref = (f - mean) @ comp
    scale = np.abs(f - mean).sum(axis=1, keepdims=True) * np.abs(comp).max() + 1e-300
    assert np.all(np.abs(o[:, D:] - ref) <= 1e-12 * scale)


def _run(args, timeout=300):
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def _read(path):
    out = {}
    for line in open(path):
        parts = line.split()
        out[parts[0]] = np.array([float(v) for v in parts[2:2 + int(parts[1])]])
    return out


def test_facade_pca_dev_matches_numpy(tmp_path):
    x = R.pca_input()
    with open(tmp_path / "x.bin", "wb") as f:  # save_betti_features layout
        f.write(np.array(x.shape, np.int32).tobytes())
        f.write(np.asfortranarray(x).tobytes(order="F"))
    out = tmp_path / "pca.txt"
    rc, _, err = _run([os.path.join(BIN, "facade_check"), "pca_dev", str(tmp_path / "x.bin"), "6", str(out)])
    assert rc == 0, err
    d = _read(out)
    comp = d["components"].reshape(35, 6, order="F")
    R.assert_model_matches_svd(x, d["mean"], comp, d["ratio"])
    np.testing.assert_allclose(d["transform"].reshape(-1, 6, order="F"), (x - x.mean(0)) @ comp, atol=1e-9)


def _load_model(path):
    raw = open(path, "rb").read()
    k, dim = np.frombuffer(raw[:8], np.int32)
    mean = np.frombuffer(raw[8:8 + 8 * dim], np.float64)
    o = 8 + 8 * dim
    r, c = np.frombuffer(raw[o:o + 8], np.int32)
    comp = np.frombuffer(raw[o + 8:o + 8 + 8 * r * c], np.float64).reshape(r, c, order="F")
    o += 8 + 8 * r * c
    kk = np.frombuffer(raw[o:o + 4], np.int32)[0]
    ratio = np.frombuffer(raw[o + 4:o + 4 + 8 * kk], np.float64)
    assert o + 4 + 8 * kk == len(raw)
    return (int(k), int(dim), int(r), int(c), int(kk)), mean, comp, ratio


def test_preprocess_driver_stream_pca(tmp_path):
    exe = os.path.join(BIN, "preprocess_betti")
    plain, plain2, stream = tmp_path / "plain", tmp_path / "plain2", tmp_path / "stream"
    for outdir, flags in ((plain, []), (plain2, []), (stream, ["--stream-pca"])):
        rc, _, err = _run([exe] + flags + [POSCARS, str(outdir), "5", "6", "4"])
        assert rc == 0, err
    bins = sorted(os.path.basename(b) for b in glob.glob(str(plain / "betti" / "*.bin")))
    assert len(bins) == len(NAMES)
    rows = []
    for b in bins:
        raw = open(plain / "betti" / b, "rb").read()
        assert raw == open(stream / "betti" / b, "rb").read(), b
        assert raw == open(plain2 / "betti" / b, "rb").read(), b
        r, c = np.frombuffer(raw[:8], np.int32)
        rows.append(np.frombuffer(raw[8:], np.float64).reshape(r, c, order="F"))
    assert open(plain / "pca_model.bin", "rb").read() == open(plain2 / "pca_model.bin", "rb").read()
    shape_p, mean_p, _, _ = _load_model(plain / "pca_model.bin")
    shape_s, mean_s, comp, ratio = _load_model(stream / "pca_model.bin")
    assert shape_s == shape_p == (6, 35, 35, 6, 6)
    np.testing.assert_allclose(mean_s, mean_p, rtol=1e-12)
    R.assert_model_gap_free(np.concatenate(rows), mean_s, comp, ratio)
    # --resume --stream-pca: the loaded features are accumulated too: the same model
    rc, _, err = _run([exe, "--resume", "--stream-pca", POSCARS, str(stream), "5", "6", "4"])
    assert rc == 0, err
    assert f"resume: {len(NAMES)} existing" in err
    shape_r, mean_r, comp_r, ratio_r = _load_model(stream / "pca_model.bin")
    assert shape_r == shape_s and np.array_equal(mean_r, mean_s) and np.array_equal(comp_r, comp)
