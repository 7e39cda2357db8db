"""CPU checks of the dense-ring inputs (tests/s1_dense_data.py) that
tests/test_gpu_s1_dense.py feeds to k_s1: the data must provably put every
twin-site row into the kernel's re-scoring ring, and the oracle on distinct
rows with multiplicities must be the oracle on the expanded rows.  No GPU.
"""
import numpy as np
import pytest

import s1_dense_data as sd
from oracle import kmeans_oracle as orc

N_CU = 256  # MI355X; the GPU tests read the device's own


def test_geometry_restates_the_kernel_constants():
    # s1_waves / s1_ring (km_screen1.hip): twelve waves and a 12-slot ring on
    # the c3 and c4 geometries only
    assert sd.geometry(64, 254) == {"dp": 64, "kp": 256, "ns2": 2, "nb": 8, "waves": 12, "ring": 12}
    assert sd.geometry(32, 1000) == {"dp": 32, "kp": 1024, "ns2": 1, "nb": 32, "waves": 12, "ring": 12}
    assert sd.geometry(64, 126)["waves"] == 8 and sd.geometry(64, 126)["ring"] == 16
    assert sd.geometry(64, 256)["waves"] == 12
    assert sd.rows_for_tiles(64, 254, N_CU, 5) == 245_767
    assert sd.rows_for_tiles(64, 126, N_CU, 5) == 163_847


def test_ring_fill_sequence_of_the_dense_rows():
    # the ring arithmetic of km_s1_ring.h on all-needy tiles: a 12-slot ring
    # completes two batches in every third tile, a 16-slot ring one per tile
    for ring, want in ((12, [(1, 4), (1, 8), (2, 0), (1, 4), (1, 8)]), (16, [(1, 0)] * 5)):
        rc, got = 0, []
        for _ in range(5):
            full, rc = divmod(rc + sd.TILE, ring)
            got.append((full, rc))
        assert got == want


def test_colouring_fills_chains_and_is_a_partition():
    ds = sd.dense(64, 254, "near")
    ch = sd.color_chains(ds.C, 8)
    assert ch.min() >= 0 and ch.max() <= 31
    assert np.bincount(ch, minlength=32).max() <= 8
    # the first 32 centroids open the 32 chains in order (empty chains first)
    np.testing.assert_array_equal(ch[:32], np.arange(32))
    # an exact duplicate of a centroid never joins its chain while another has room
    C = np.concatenate([ds.C[:40], ds.C[:1]])
    assert sd.color_chains(C, 8)[40] != 0


@pytest.mark.parametrize("d,k,pattern,kind,n_single", [
    (64, 254, 8, "exact", 0), (64, 254, 8, "ulp", 0), (64, 254, 8, "near", 0),
    (32, 1000, 4, "exact", 0), (32, 1000, 4, "near", 0),
    (64, 254, 8, "exact", 18), (64, 254, 8, "near", 18),
    (64, 126, 8, "exact", 0), (64, 126, 8, "near", 0),
])
def test_predict_inputs_meet_the_ring_preconditions(d, k, pattern, kind, n_single):
    ds = sd.dense(d, k, kind, n_single, pattern=pattern)
    assert ds.C.shape == (k, d) and np.array_equal(ds.U, ds.U.astype(np.float32))
    m = sd.check_ring_rows(ds)
    assert m["twin_gap_over_E"] <= 0.25 and m["rest_over_E"] >= 8.0
    # near twins share their site's rows; of exact duplicates the lower index
    # takes them all; one-ulp duplicates are told apart in float64 only
    lab = orc.assign(ds.U, ds.C, chunk=sd.ORACLE_CHUNK)[0]
    tw = ds.twin_rows
    assert np.all(lab[~tw] == 2 * ds.St + (ds.site[~tw] - ds.St))
    assert np.all((lab[tw] == ds.site[tw]) | (lab[tw] == ds.St + ds.site[tw]))
    if kind == "near":
        assert 0.2 < np.mean(lab[tw] == ds.site[tw]) < 0.8
    elif kind == "exact":
        assert np.all(lab[tw] == ds.site[tw])
    inverse = sd.expand(len(ds.U), 10_007, seed=1)
    cnt = np.bincount(inverse, minlength=len(ds.U))
    assert cnt.max() - cnt.min() <= 1 and np.sum(cnt[0::2] != cnt[1::2]) <= 1


def test_a_violated_precondition_is_caught():
    # twins 4 apart: their scores differ by far more than E / 4
    ds = sd.dense(64, 62, "near")
    C = ds.C.copy()
    C[ds.St:2 * ds.St] = ds.G[:ds.St] + 4.0 * ds.e[:ds.St]
    with pytest.raises(AssertionError):
        sd.check_ring_rows(ds, C)


@pytest.mark.parametrize("d,k,pattern", [(64, 254, 8), (32, 1000, 4)])
def test_fit_inputs_keep_moving_and_stay_ring_rows(d, k, pattern):
    # precondition (e) at the GPU tests' size on a 256-CU part
    ds, C0, inverse, ref, info = sd.fit_case(d, k, n=sd.rows_for_tiles(d, k, N_CU, 5), pattern=pattern)
    assert sum(m >= 0.05 for m in info["moved"]) >= 2
    for m in info["margins"]:
        assert m["twin_gap_over_E"] <= 0.25 and m["rest_over_E"] >= 8.0 and m["near_gap_over_width"] >= 10.0
    # the twins stay about delta apart
    for C in ref["centroids"]:
        gap = np.linalg.norm(C[:ds.St] - C[ds.St:2 * ds.St], axis=1)
        assert np.all((gap > 0.5 * ds.delta) & (gap < 2.5 * ds.delta))


def test_weighted_lloyd_equals_the_oracle_on_expanded_rows():
    d, k, iters = 64, 62, 4
    ds, C0, inverse, ref, _ = sd.fit_case(d, k, iters=iters, n=2003)
    X = ds.U[inverse]
    full = orc.lloyd_fit(X, k, iters, 1e-12, 0, True, 1, init_centroids=C0)
    assert full["n_iter"] == iters and not any(r["empty"] for r in full["records"])
    np.testing.assert_allclose(ref["centroids"][iters], full["centroids"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["sse_history"], full["sse_history"], rtol=1e-12)
    for i in range(iters):
        np.testing.assert_array_equal(ref["labels"][i][inverse], orc.assign(X, ref["centroids"][i])[0])
        assert full["records"][i]["sizes"] == ref["counts"][i].tolist()
