"""Morph targets in the host mirror (cgpth_morph_triangles; csrc/host/morph.h) against their numpy statement and their float64 model
(tests/morph_ref.py), CPU only.  The device kernel is held to the same mirror in tests/test_gpu_morph.py."""
import numpy as np
import pytest

import cpugpupathtracing_amd as P
from morph_cases import CASES, FLATTEN_EVERY, ZEROS_AMONG_W, make_case, planted
from morph_ref import U, component_bound, gamma, morph_f32, morph_f64, normal_bound
from scenes import GROUND_I, GROUND_V, standin_mesh
from skin_cases import make_case as skin_case, strip_mesh
from skin_ref import skin_f32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def meshes():
    return {"standin": P.triangles_from_arrays(*standin_mesh(2)), "ground": P.triangles_from_arrays(GROUND_V, GROUND_I),
            "strip": P.triangles_from_arrays(*strip_mesh(257)), "one": P.triangles_from_arrays(*strip_mesh(1))}


def cases_of(name, meshes):
    for mesh, tris in meshes.items():
        if name == "limit" and mesh == "standin":
            continue                                                          # 256 targets on the small meshes only
        yield (mesh,) + make_case(name, tris, seed=3)


@pytest.mark.parametrize("name", CASES)
def test_mirror_equals_the_float32_statement_bit_for_bit(meshes, name):
    for mesh, base, d, w in cases_of(name, meshes):
        got = P.morph_triangles(base, d, w)
        want = morph_f32(base, d, w)
        assert got.shape == base.shape and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want)), f"{mesh}: {np.count_nonzero(bits(got) != bits(want))} words differ"
        assert np.array_equal(bits(got), bits(base)) == (name == "all_zero")   # no active target: the base bytes; else something moved


@pytest.mark.parametrize("name", CASES)
def test_mirror_is_within_the_forward_error_of_the_float64_model(meshes, name):
    checked = 0
    for mesh, base, d, w in cases_of(name, meshes):
        k = w.size
        got = P.morph_triangles(base, d, w).reshape(-1, 3, 6).astype(np.float64)
        pos, unit, length, s_p, s_n = morph_f64(base, d, w)
        err_p = np.abs(got[..., :3] - pos)
        assert (err_p <= component_bound(s_p, k)).all(), (mesh, float((err_p / np.maximum(component_bound(s_p, k), 1e-300)).max()))
        bound_n, rel = normal_bound(s_n, length, k)
        ok = rel <= 0.1                                                        # where the blended normal is not about to vanish
        # The mask leaves out at most 1 % of the corners, on every case and mesh but one: `flatten` cancels the normal of corner 0 of every
        # mesh on purpose (and of every 128th corner after it), which on the two meshes of 6 and 3 corners is 1 corner in 6 and 1 in 3.
        # There exactly that one corner is masked.
        if name == "flatten" and mesh in ("ground", "one"):
            assert (~ok).sum() == 1 and not ok.reshape(-1)[0]
        else:
            assert 1.0 - ok.mean() <= 0.01, (name, mesh, float(ok.mean()))
        if name == "all_zero":                                                # the base normals as given: unit to float32 only
            assert np.array_equal(bits(got.astype(np.float32)), bits(base.reshape(-1, 3, 6)))
            continue
        err_n = np.abs(got[..., 3:] - unit).max(axis=-1)
        assert (err_n[ok] <= bound_n[ok]).all(), (mesh, float((err_n[ok] / bound_n[ok]).max()))
        assert np.allclose(np.linalg.norm(got[..., 3:][ok], axis=-1), 1.0, atol=1e-6)
        checked += int(ok.sum())
    assert checked > 700 or name == "all_zero"
    assert gamma(257) < 258 * U * 1.0001


def test_the_skip_of_zero_weights_is_observable(meshes):
    base, d, w = make_case("zeros_among", meshes["standin"], seed=3)
    assert np.array_equal(bits(w), bits(ZEROS_AMONG_W)) and (np.signbit(w) & (w == 0)).any() and (~np.signbit(w) & (w == 0)).any()
    t, f = planted(base.shape[0])
    assert len(t) > 100 and np.signbit(base[t, f]).all() and (base[t, f] == 0).all()
    got = P.morph_triangles(base, d, w)
    assert np.signbit(got[t, f]).all() and (got[t, f] == 0).all()             # -0.0 survives the four skipped targets
    x = base.copy()
    for k in range(w.size):                                                   # the statement without the skip
        x = x + w[k] * d[k]
    assert not np.signbit(x[t, f]).any()                                      # ... which it would not have


def test_normals_that_cancel_keep_the_base_normal(meshes):
    for mesh in ("standin", "one"):
        base, d, w = make_case("flatten", meshes[mesh], seed=3)
        got = P.morph_triangles(base, d, w).reshape(-1, 6)
        b = base.reshape(-1, 6)
        c = np.arange(0, b.shape[0], FLATTEN_EVERY)
        assert np.array_equal(bits(got[c, 3:]), bits(b[c, 3:]))               # kept, bit for bit
        assert not np.array_equal(got[c, :3], b[c, :3])                       # while the positions moved
        rest = np.setdiff1d(np.arange(b.shape[0]), c)
        if rest.size:
            assert np.allclose(np.linalg.norm(got[rest, 3:], axis=-1), 1.0, atol=1e-6)


def test_a_pose_is_computed_from_the_base(meshes):
    tris = meshes["standin"]
    base, d, _ = make_case("mix", tris)
    wa, wb = np.float32([-0.5, 0.25, 1.75]), np.float32([1.0, 0.0, -2.0])
    a1 = P.morph_triangles(base, d, wa)
    b1 = P.morph_triangles(base, d, wb)
    a2 = P.morph_triangles(base, d, wa)
    assert np.array_equal(bits(a1), bits(a2)) and not np.array_equal(bits(a1), bits(b1))
    assert np.array_equal(base, tris)                                         # the input is not written


def test_morph_then_skin_is_the_composition_of_the_two_statements(meshes):
    """what the fused device pose is held to: skin_triangles with the morphed triangles as its bind pose"""
    for mesh in ("standin", "strip", "one"):
        base, d, w = make_case("mix", meshes[mesh], seed=7)
        j, sw, n_joints, m = skin_case("four", base, seed=7)
        got = P.skin_triangles(P.morph_triangles(base, d, w), j, sw, m)
        want = skin_f32(morph_f32(base, d, w), j, sw, m)
        assert np.array_equal(bits(got), bits(want))
        assert not np.array_equal(bits(got), bits(P.skin_triangles(base, j, sw, m)))
        zero = P.skin_triangles(P.morph_triangles(base, d, np.zeros(3, np.float32)), j, sw, m)
        assert np.array_equal(bits(zero), bits(P.skin_triangles(base, j, sw, m)))   # no active target: the plain skin
