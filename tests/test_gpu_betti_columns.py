"""The narrow Betti kernels' rank-ordered column walk (csrc/betti_kernels.hip, reduce_serial): the
non-apparent columns of a dimension sit in registers in Ripser's column order, only the columns
that can need an addition are walked, and pairs, counts and clearing marks are written lane-parallel
after the walk.

  * DGN_DEBUG_NARROW_VISIT_ALL (every column walked) against the default, byte for byte: pairs in
    emission order, counts and the 35 features, through host_persistence[_lower], host_betti and
    dev_graph_betti;
  * the same inputs against verbatim Ripser (the restated oracle where oracle/_ref is not built),
    as sorted multisets;
  * DGN_DEBUG_FORCE_RETRY on one mixed batch: a complex whose walk stops on a full workspace must
    leave the scratch state the capacity-retry launch and the next complex expect.

The column census (dgn_debug_column_stats) shows that the inputs skip columns, promote columns and
take the path of more than 128 columns."""
import numpy as np
import pytest
import torch

import dgn
import oracle_py as O
from dgn import abi

pytestmark = pytest.mark.gpu
CAP = 4096


def _ref(low, n, thr):
    return O.ref_persistence(low, n, thr) if O.ref_available() else O.persistence(low, n, thr)


def _sphere(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _cube_clouds(seed):
    """Uniform clouds of 12, 33, 48, 49 and 64 points in a 5 A cube (two of each size)."""
    rng = np.random.default_rng(seed)
    sizes = [12, 33, 48, 49, 64] * 2
    clouds = np.zeros((len(sizes), 64, 3))
    for c, n in enumerate(sizes):
        clouds[c, :n] = rng.uniform(0.0, 5.0, size=(n, 3))
    return clouds, np.array(sizes, np.int32)


def _sphere_clouds(seed, count=4):
    rng = np.random.default_rng(seed)
    return np.stack([_sphere(rng, 40) for _ in range(count)]), np.full(count, 40, np.int32)


def _lower_of(clouds, npts):
    maxp = clouds.shape[1]
    low = np.zeros((len(npts), maxp * (maxp - 1) // 2), np.float32)
    for c, n in enumerate(npts):
        low[c, :n * (n - 1) // 2] = O.local_distances(clouds[c, :n])
    return low


class _Set:
    def __init__(self, name, lower, npts, thr, batch=None):
        self.name, self.lower, self.npts, self.thr, self.batch = name, lower, npts, np.float32(thr), batch
        self.maxp = int(round((1 + np.sqrt(1 + 8 * lower.shape[1])) / 2))


@pytest.fixture(scope="module")
def runs(ctx):
    """Every input set reduced twice (default walk, every column walked): pairs, counts and the
    default walk's column census, computed once for the tests below."""
    sets = []
    for name, kind, count in (("fcc256", "fcc", 2), ("sc64", "sc", 64)):
        batch = dgn.synth_batch(kind, 4, count)
        A = batch["positions"].shape[0]
        lower, npts, _ = ctx.debug_betti_clouds(batch, 5.0, 0, A, 64)
        sets.append(_Set(name, lower, npts, 5.0, batch))
    cube, cn = _cube_clouds(101)
    for thr in (1.5, 1.9, 2.4):
        sets.append(_Set(f"cube@{thr}", _lower_of(cube, cn), cn, thr))
    sph, sn = _sphere_clouds(103)
    for thr in (0.8, 2.0):
        sets.append(_Set(f"sphere@{thr}", _lower_of(sph, sn), sn, thr))
    out = {}
    ctx.set_debug(abi.DEBUG_COLUMN_STATS, 1)
    try:
        for s in sets:
            ctx.column_stats()
            p0, c0 = ctx.host_persistence_lower(s.lower, s.npts, s.maxp, float(s.thr), cap=CAP)
            census = ctx.column_stats()
            ctx.set_debug(abi.DEBUG_NARROW_VISIT_ALL, 1)
            try:
                p1, c1 = ctx.host_persistence_lower(s.lower, s.npts, s.maxp, float(s.thr), cap=CAP)
                census_all = ctx.column_stats()
            finally:
                ctx.set_debug(abi.DEBUG_NARROW_VISIT_ALL, 0)
            out[s.name] = dict(set=s, pairs=p0, counts=c0, pairs_all=p1, counts_all=c1, census=census,
                               census_all=census_all)
    finally:
        ctx.set_debug(abi.DEBUG_COLUMN_STATS, 0)
    return out


NAMES = ["fcc256", "sc64", "cube@1.5", "cube@1.9", "cube@2.4", "sphere@0.8", "sphere@2.0"]


@pytest.mark.parametrize("name", NAMES)
def test_visit_all_pairs_byte_for_byte(runs, name):
    r = runs[name]
    assert np.array_equal(r["counts"], r["counts_all"]), name
    assert r["counts"].min() >= 0, name
    assert np.array_equal(r["pairs"].view(np.uint32), r["pairs_all"].view(np.uint32)), name
    # walking every column skips none and promotes none
    assert r["census_all"]["skipped"] == 0 and r["census_all"]["promoted"] == 0, r["census_all"]
    assert r["census_all"]["walked"] == r["census"]["walked"] + r["census"]["skipped"], (r["census"], r["census_all"])


def test_census_over_the_batch(runs):
    """The inputs make the walk skip columns, promote later columns and cross 128 columns."""
    tot = {k: sum(r["census"][k] for r in runs.values()) for k in ("skipped", "walked", "promoted", "spilled")}
    print("column census:", {n: r["census"] for n, r in runs.items()})
    assert tot["skipped"] > 0 and tot["walked"] > 0 and tot["promoted"] > 0 and tot["spilled"] > 0, tot


@pytest.mark.parametrize("name", NAMES)
def test_pairs_vs_ripser(runs, name):
    r = runs[name]
    s, pairs, counts = r["set"], r["pairs"], r["counts"]
    bad = []
    for c in range(len(s.npts)):
        n = int(s.npts[c])
        ref = _ref(s.lower[c, :n * (n - 1) // 2], n, s.thr)
        assert max(len(ref[d]) for d in ("dim0", "dim1", "dim2")) <= CAP
        got = {"dim0": pairs[c, 0, :counts[c, 0]], "dim1": pairs[c, 1, :counts[c, 2]], "dim2": pairs[c, 2, :counts[c, 3]]}
        ok = all(np.array_equal(np.array(sorted(map(tuple, got[d]))).reshape(-1, 2), ref[d].reshape(-1, 2))
                 for d in got) and counts[c, 1] == ref["n_inf0"]
        if not ok:
            bad.append((c, n, counts[c].tolist(), [len(ref[d]) for d in ("dim0", "dim1", "dim2")], ref["n_inf0"]))
    assert not bad, (name, bad[:8])


def _features(ctx, batch):
    """(features, counts) of a structure batch through host_betti and through dev_graph_betti."""
    f, c = ctx.host_betti(batch, 5.0)
    dev = torch.device("cuda", 0)
    db = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    A = batch["positions"].shape[0]
    gp = abi.graph_params(r_cutoff=5.0, max_neighbors=20, rbf_cutoff=5.0, rbf_dr=0.1, rbf_dtype=dgn.DGN_F32)
    nb = abi.lib().dgn_rbf_bins(5.0, 0.1)
    E = ctx.dev_graph_count(db, gp)
    rp = torch.empty(A + 1, dtype=torch.int64, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    dist = torch.empty(E, dtype=torch.float64, device=dev)
    rbf = torch.empty((E, nb), dtype=torch.float32, device=dev)
    feat = torch.zeros((A, 35), dtype=torch.float64, device=dev)
    cnt = torch.zeros((A, 4), dtype=torch.int32, device=dev)
    ctx.dev_graph_betti(db, gp, rp, col, dist, None, rbf, 5.0, feat, cnt)
    ctx.synchronize()
    return f, c, feat.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("name", ["fcc256", "sc64"])
def test_visit_all_features_byte_for_byte(ctx, runs, name):
    batch = runs[name]["set"].batch
    off = _features(ctx, batch)
    ctx.set_debug(abi.DEBUG_NARROW_VISIT_ALL, 1)
    try:
        on = _features(ctx, batch)
    finally:
        ctx.set_debug(abi.DEBUG_NARROW_VISIT_ALL, 0)
    for a, b in zip(off, on):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    # both entry points, and the pair counts of the pair-list entry point
    assert np.array_equal(off[0].view(np.uint64), off[2].view(np.uint64)), name
    assert np.array_equal(off[1], off[3]) and np.array_equal(off[1], runs[name]["counts"]), name


def test_forced_retry_mixed_batch(ctx):
    """Cube clouds of every narrow tier beside 40-point cliques on the sphere (their walks stop on
    a full V list): every complex through the capacity-retry launch, then the same batch again
    without the knob on the scratch the first pass left."""
    cube, cn = _cube_clouds(107)
    sph, sn = _sphere_clouds(109, 2)
    clouds = np.zeros((len(cn) + len(sn), 64, 3))
    clouds[:len(cn)] = cube
    clouds[len(cn):, :40] = sph
    npts = np.concatenate([cn, sn])
    order = np.random.default_rng(113).permutation(len(npts))
    clouds, npts = clouds[order], npts[order]
    lower = _lower_of(clouds, npts)
    refs = [_ref(lower[c, :n * (n - 1) // 2], int(n), np.float32(2.0)) for c, n in enumerate(npts)]

    def check(forced):
        ctx.retry_count()
        pairs, counts = ctx.host_persistence_lower(lower, npts, 64, 2.0, cap=1 << 15)
        kt = ctx.retry_count()
        for c, ref in enumerate(refs):
            got = {"dim0": pairs[c, 0, :counts[c, 0]], "dim1": pairs[c, 1, :counts[c, 2]], "dim2": pairs[c, 2, :counts[c, 3]]}
            for d in got:
                assert np.array_equal(np.array(sorted(map(tuple, got[d]))).reshape(-1, 2), ref[d].reshape(-1, 2)), \
                    (forced, c, int(npts[c]), d)
            assert counts[c, 1] == ref["n_inf0"], (forced, c)
        return kt

    ctx.set_debug(abi.DEBUG_FORCE_RETRY, 1)
    try:
        kt = check(True)
    finally:
        ctx.set_debug(abi.DEBUG_FORCE_RETRY, 0)
    assert kt >= len(npts), kt
    check(False)
