"""The MFMA path (path 2) on rows and centroids at the edges of the float32
range, against the float64 oracle: every dispatch class, from 1e-30 to 1e20.

The screens work in scaled units (a power of two s brings max(|x|, |c|) into
[2^13, 2^14)), so ordinary float32 data of any magnitude should be screened
like data near 1 -- provided every quantity that enters a scaled bound is
scaled before it is rounded to fp32.  ||c||^2 and max ||c|| were not: at
1e-25 the accumulator seed ||c||^2 s^2 was 0 and max ||c|| was 1e-30 where it
is 1e-24, and the norm term decides most labels of these inputs
(tests/range_data.py; tests/test_host_range_data.py checks, without a GPU,
that they are what these tests assume).

a. scale sweep: one step (compute_sse on and off, both sweep directions) on
   every dispatch class, with the default screen and with each forced one,
   and a predict pass (k_s1 MODE 0) where the class has it;
b. three iterations at engine level (k_s1 in delta mode, its SSE form with the
   update's correction, k_s1_delta, the update's own max ||c||);
c. the row gate's scale range s in [2^-30, 2^30], the same rows on both sides;
d. mixed magnitudes: one huge row, one huge centroid, tiny rows beside
   ordinary ones, denormal rows.
"""
import numpy as np
import pytest

import range_data as rd
from test_gpu_small_instances import _check_step, _load, _step

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(key, X, C0, iters=1):
    """The oracle's steps for an input, computed once and left unchanged."""
    if key not in _refs:
        out = rd.lloyd(X, C0, iters)
        for r in out:
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _geo(name, **more):
    _, _, _, dp, kp, fused, _ = rd.CLASSES[name]
    return dict(path=2, dp=dp, kp=kp, fused=fused, **more)


def _atol(X):
    return 1e-9 * float(np.abs(X).max())


# ----------------------------------------------------------------- a. scale sweep
@pytest.mark.parametrize("scale", rd.SCALES)
@pytest.mark.parametrize("name", list(rd.CLASSES))
def test_scale_sweep_one_step(name, scale):
    X, C0 = rd.class_case(name, scale)
    ref = _ref((name, scale), X, C0)[0]
    for sse in (True, False):
        out = _step(X, C0, sse, **_geo(name))
        print(f"{name} scale {scale:g} sse {sse}: queued {out['q']} of {len(X)}")
        _check_step(out, ref, sse, atol=_atol(X))
        if scale == 1.0:   # the control: the screen, not the float64 resolver, is under test
            assert out["q"] < len(X) / 4


# 0: plain fp16x3; 1: fp16x3 with per-key bounds; 5: one MFMA per product;
# 4: k_s1.  A mode the geometry has no kernel for leaves the default in place
SCREENS = [0, 1, 5, 4]


@pytest.mark.parametrize("scale", rd.SCALES)
@pytest.mark.parametrize("name", list(rd.CLASSES))
def test_scale_sweep_forced_screens(name, scale):
    X, C0 = rd.class_case(name, scale)
    ref = _ref((name, scale), X, C0)[0]
    for i, mode in enumerate(SCREENS):
        sse = bool((i + (scale > 1)) % 2)   # both forms of every mode over the sweep
        out = _step(X, C0, sse, sweeps=1, **_geo(name, screen=mode))
        print(f"{name} scale {scale:g} screen {mode} sse {sse}: queued {out['q']} of {len(X)}")
        _check_step(out, ref, sse, atol=_atol(X))


@pytest.mark.parametrize("scale", rd.SCALES)
@pytest.mark.parametrize("name", rd.PREDICT_CLASSES)
def test_scale_sweep_predict(name, scale):
    X, C0 = rd.class_case(name, scale)
    ref = _ref((name, scale), X, C0)[0]
    eng = _load(X, C0, False, **_geo(name))
    # (labels only: k_s1 MODE 0 wherever the geometry has an instance, which
    # dp and kp, asserted above, decide)
    for _ in range(2):
        np.testing.assert_array_equal(eng.predict(), ref["labels"])
    eng.close()


# ------------------------------------------------------------ b. three iterations
def _iterations(X, C0, sse, refs, **geo):
    """assign_stats / update / commit as the driver runs them; each
    iteration's labels, counts, centroids and SSE against the oracle's.
    Returns the rows each pass screened (km_gated_rows)."""
    eng = _load(X, C0, sse, **geo)
    atol = _atol(X)
    gated = []
    for i, ref in enumerate(refs):
        eng.assign_stats()
        st, cnt = eng.update()
        gated.append(eng.info()["gated_rows"])
        np.testing.assert_array_equal(eng.labels(), ref["labels"])
        np.testing.assert_array_equal(cnt, ref["counts"])
        assert st.n_empty == 0 and st.nonfinite == 0
        np.testing.assert_allclose(eng.get_centroids(1), ref["new"], rtol=1e-9, atol=atol)
        if sse:
            print(f"iteration {i + 1}: sse {st.sse!r} vs {ref['sse']!r}")
            np.testing.assert_allclose(st.sse, ref["sse"], rtol=1e-9)
        if i + 1 < len(refs):
            eng.commit()
    delta = eng.info()["delta_stats"]
    eng.close()
    return gated, delta


@pytest.mark.parametrize("sse", [True, False])
@pytest.mark.parametrize("scale", rd.ITER_SCALES)
@pytest.mark.parametrize("name", rd.ITER_CLASSES)
def test_three_iterations(name, scale, sse):
    X, C0 = rd.class_case(name, scale)
    refs = _ref((name, scale, "iter"), X, C0, rd.ITERS)
    gated, delta = _iterations(X, C0, sse, refs, **_geo(name))
    print(f"{name} scale {scale:g}: gated rows {gated}, delta statistics {delta}")
    if name in ("A", "E"):
        assert delta == 1            # k_s1 ran in delta mode
    if name == "A" and not sse:
        # these scales are outside the row gate's range: it is off (-1) or
        # screens every row
        s = rd.s1_scale(np.abs(X).max(), np.abs(C0).max())
        assert not 2.0 ** -30 <= s <= 2.0 ** 30
        assert all(g in (-1, len(X)) for g in gated), gated


# ------------------------------------------------------------ c. gate scale range
@pytest.mark.parametrize("inside,outside", rd.GATE_PAIRS)
def test_gate_scale_boundary(inside, outside):
    got = {}
    for side in (inside, outside):
        X, C0 = rd.gate_scale(side)
        refs = _ref(("gate", side), X, C0, rd.ITERS)
        got[side] = _iterations(X, C0, False, refs, **_geo("A"))[0]
    print(f"gated rows: {got}")
    for a, b in zip(_refs[("gate", inside)], _refs[("gate", outside)]):
        np.testing.assert_array_equal(a["labels"], b["labels"])
    n = rd.CLASSES["A"][0]
    assert 0 <= got[inside][-1] < n
    assert got[outside][-1] in (-1, n)


# ------------------------------------------------------------ d. mixed magnitudes
@pytest.mark.parametrize("name", rd.MIXED_CLASSES)
@pytest.mark.parametrize("kind", list(rd.MIXED))
def test_mixed_magnitudes(kind, name):
    X, C0 = rd.mixed_case(kind, name)
    ref = _ref((kind, name), X, C0)[0]
    out = _step(X, C0, True, **_geo(name))
    print(f"{kind} {name}: queued {out['q']} of {len(X)}")
    _check_step(out, ref, True, atol=_atol(X))
    assert out["n_empty"] == (1 if kind == "outlier_centroid" else 0)
