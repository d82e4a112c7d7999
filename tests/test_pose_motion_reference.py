"""The numpy statement of CGPT_TEMPORAL_FOLLOW_POSES (pose_motion_ref.py) against closed forms, and how many pixels a float32 run of
the statement decides differently on the scene and the pose changes of the device tests (pose_motion_cases.py).  No GPU."""
import numpy as np
import pytest

import denoise_ref as D
import motion_ref as M
import pose_motion_cases as PC
import pose_motion_ref as PM
import skin_cases as SC
import transform_scenes as TS
import cpugpupathtracing_amd as P
from test_temporal_reference import PH, PW, frame, plane_camera, plane_guides, random_acc

IDENTITY = np.eye(3, 4, dtype=np.float32)
# the card of test_motion_reference.py as a skinned quad: two triangles over x in [-2, 2), y in [-10, 10] on the wall z = 0, one joint
QUAD = np.float32([[-2, -10, 0, 0, 0, 1, 2, -10, 0, 0, 0, 1, 2, 10, 0, 0, 0, 1], [-2, -10, 0, 0, 0, 1, 2, 10, 0, 0, 0, 1, -2, 10, 0, 0, 0, 1]])
QUAD_J = np.zeros((2, 3, 4), np.uint16)
QUAD_W = np.zeros((2, 3, 4), np.float32)
QUAD_W[..., 0] = 1.0


def shifted(dx, dy=0.0, dz=0.0):
    return SC.matrix(b=(dx, dy, dz)).reshape(1, 12)


def card(matrices, serial=1):
    return {1: PM.Posed(QUAD, QUAD_J, QUAD_W, matrices, serial)}


def card_guides(cx, card_x):
    """plane_guides with the card, object 1, over world x in [card_x - 2, card_x + 2); (guides, the card's pixels, triangle indices)"""
    g = plane_guides(cx)
    on = (g[..., 0] >= card_x - 2.0) & (g[..., 0] < card_x + 2.0)
    g.view(np.uint32)[on, 7] = 1
    local = g[..., 0:2].astype(np.float64) - [card_x, 0.0]
    tri = np.where(on & (local[..., 1] + 10.0 > 5.0 * (local[..., 0] + 2.0)), 1, 0).astype(np.uint32)   # above the diagonal: triangle 1
    return g, on, tri


def random_hits(rows, rng, k=400):
    """k points on random triangles of `rows` (n, 18): (tri (k,), points (k, 3) float32)"""
    tau = rng.integers(0, rows.shape[0], k)
    u, v = rng.uniform(0, 1, k), rng.uniform(0, 1, k)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    r = rows[tau].astype(np.float64)
    return tau, (r[:, 0:3] + u[:, None] * (r[:, 6:9] - r[:, 0:3]) + v[:, None] * (r[:, 12:15] - r[:, 0:3])).astype(np.float32)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------

def test_a_rigid_one_joint_pose_is_the_transform_carry_back_with_the_same_matrix():
    rng = np.random.default_rng(31)
    bind = P.triangles_from_arrays(*TS.box_mesh((-1.4, -1.0, -1.2), (1.4, 1.2, 0.8)))
    n = bind.shape[0]
    j, w = np.zeros((n, 3, 4), np.uint16), np.zeros((n, 3, 4), np.float32)
    w[..., 0] = 1.0
    prev = SC.matrix(SC.rotation((0.2, 1.0, 0.3), 25.0), (0.3, 0.2, -0.4)).reshape(1, 12)
    cur = SC.matrix(SC.rotation((1.0, 0.1, -0.4), -40.0), (-0.8, 0.5, 0.2)).reshape(1, 12)
    posed = PM.Posed(bind, j, w, cur)
    tau, x = random_hits(posed.triangles(), rng)
    x_p, n_p, ok = PM.carry_hits(x, tau, posed, prev)
    assert ok.all()
    rec = M.motion_record(prev, cur).view(np.float32).reshape(6, 4).astype(np.float64)
    want = x.astype(np.float64) @ rec[:3, :3].T + rec[:3, 3]
    rel = np.max(np.abs(x_p - want)) / np.max(np.abs(want))
    print(f"rigid pose against D x: {rel:.2e} relative")
    assert rel <= 1e-6
    flat = posed.triangles()[tau, 3:6].astype(np.float64)                      # the current flat normal, carried back by N
    nw = flat @ rec[3:, :3].T
    assert np.max(np.abs(n_p - nw / np.linalg.norm(nw, axis=1, keepdims=True))) <= 1e-6


def test_a_hit_at_a_corner_maps_to_the_history_corner_exactly():
    bind = PC.bind_triangles()[PC.MOVER]
    j, w, _, m = SC.make_case("bend", bind, seed=3)
    prev = PC.varied(m, bind, 4.0, (0.3, -0.2, 0.1))
    posed = PM.Posed(bind, j, w, m)
    cur, hist = posed.triangles(), posed.triangles(prev)
    tau = np.arange(bind.shape[0])
    for c in range(3):
        x_p, _, ok = PM.carry_hits(cur[:, 6 * c:6 * c + 3], tau, posed, prev)  # u, v in {0, 1}
        assert ok.all() and np.array_equal(x_p.view(np.uint32), hist[:, 6 * c:6 * c + 3].view(np.uint32)), c


def test_a_pose_that_shifts_by_whole_pixels_takes_its_history_shifted_and_the_background_its_own():
    rng = np.random.default_rng(32)
    cam = plane_camera()
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    g1, on1, t1 = card_guides(0.0, -1.0)
    g2, on2, t2 = card_guides(0.0, 2.0)                                        # three world units = three pixels to the right
    m = PM.Temporal()
    out1, _ = frame(m, a1, 4, g1, cam, tri=t1, posed=card(shifted(-1.0)), follow_poses=True)
    out2, _ = frame(m, a2, 1, g2, cam, tri=t2, posed=card(shifted(2.0)), follow_poses=True)
    c2 = D.radiance(a2, 1).astype(np.float64)
    cols1, cols2 = np.flatnonzero(on1[0]), np.flatnonzero(on2[0])
    assert list(cols2 - cols1) == [3] * 4 and set(np.unique(t2[on2])) == {0, 1}
    Hn = m.history[..., 3]
    assert np.all(PM.record_states(m.records)[on2] == PM.REPOSED) and np.all(PM.record_states(m.records)[~on2] == PM.UNPOSED)
    assert np.all(Hn[:, cols2] == 5)
    assert np.allclose(out2[:, cols2, :3], (4 * out1[:, cols1, :3] + c2[:, cols2]) / 5, rtol=1e-12, atol=0)
    never = ~on1[0] & ~on2[0]
    assert np.all(Hn[:, never] == 5)
    assert np.allclose(out2[:, never, :3], (4 * out1[:, never, :3] + c2[:, never]) / 5, rtol=1e-12, atol=0)
    revealed = on1[0] & ~on2[0]                                                # the wall the card uncovered: H' = N and c_0's bits
    assert revealed.sum() == 3
    assert np.all(Hn[:, revealed] == 1) and np.array_equal(out2[:, revealed, :3], c2[:, revealed])
    m = PM.Temporal()                                                          # without the flag the pose drops everything
    frame(m, a1, 4, g1, cam, tri=t1, posed=card(shifted(-1.0)))
    out, _ = frame(m, a2, 1, g2, cam, tri=t2, posed=card(shifted(2.0)))
    assert np.all(m.history[..., 3] == 1) and np.array_equal(out[..., :3], c2)


def test_a_b_a_is_unposed_and_the_frame_is_the_unflagged_one():
    rng = np.random.default_rng(33)
    a1, a2 = random_acc(rng, 2), random_acc(rng, 3)
    g, on, tri = card_guides(0.0, 1.0)
    cams = (plane_camera(0.0), plane_camera(0.3))
    assert PM.pose_state(card(shifted(1.0))[1].key(), card(shifted(1.0))[1].key()) == PM.UNPOSED
    assert PM.pose_state(card(shifted(1.0))[1].key(), card(shifted(2.0))[1].key()) == PM.REPOSED
    mp, mm = PM.Temporal(), M.Temporal()
    for acc, n, cam in ((a1, 2, cams[0]), (a2, 3, cams[1])):                   # B happened between the two calls; the second sees A again
        got = frame(mp, acc, n, g, cam, tri=tri, posed=card(shifted(1.0)), follow_poses=True)
        want = frame(mm, acc, n, g, cam)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(mp.history, mm.history)
    assert mp.records is None and np.mean(mp.history[..., 3] == 5) > 0.8


def test_no_pose_known_drops_that_objects_pixels_only():
    rng = np.random.default_rng(34)
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    g, on, tri = card_guides(0.0, 1.0)
    for before, after in ((None, shifted(1.0)), (shifted(1.0), None)):
        assert PM.pose_state(card(before)[1].key(), card(after)[1].key()) == PM.DROP
        m = PM.Temporal()
        frame(m, a1, 4, g, plane_camera(0.0), tri=tri, posed=card(before), follow_poses=True)
        frame(m, a2, 1, g, plane_camera(0.25), tri=tri, posed=card(after), follow_poses=True)
        Hn = m.history[..., 3]
        assert np.all(PM.record_states(m.records)[on] == PM.DROP) and np.all(Hn[on] == 1)
        assert np.mean(Hn[~on] == 5) > 0.8
    assert PM.pose_state(card(shifted(1.0), 1)[1].key(), card(shifted(2.0), 2)[1].key()) == PM.DROP     # another installation of the skin
    assert PM.pose_state(card(shifted(1.0))[1].key(), card(np.concatenate([shifted(1.0)] * 2))[1].key()) == PM.DROP   # another joint count


def test_a_degenerate_current_triangle_drops_the_pixel():
    bind = QUAD.copy()
    j, w = QUAD_J, QUAD_W
    flat = np.float32([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]).reshape(1, 12)  # the current pose collapses x: g . g = 0
    posed = PM.Posed(bind, j, w, flat)
    _, _, ok = PM.carry_hits(np.float32([[0.0, 1.0, 0.0]]), [0], posed, shifted(1.0))
    assert not ok.any()


# ---- a float32 run of the statement on the device tests' scene and pose changes ----------------------------------------------------------

@pytest.fixture(scope="module")
def host_frames():
    """per case: (guides, tri, camera, posed objects) before and after the pose change, from hits made on the host"""
    s = PC.product_scene()
    out = {}
    before = {}
    for case in PC.CASES:
        sk, base, after, view = PC.case_poses(case)
        mover = PC.CASES[case][3]
        if mover not in before:
            cam0 = PC.camera(s, PC.BASE)
            before[mover] = PC.host_guides(cam0, sk, base) + (PM.T.camera_array(cam0),)
        cam1 = PC.camera(s, view)
        g1, t1 = PC.host_guides(cam1, sk, after)
        out[case] = (before[mover], (g1, t1, PM.T.camera_array(cam1)), sk, base, after)
    return out


@pytest.mark.parametrize("back", [False, True])
@pytest.mark.parametrize("case", list(PC.CASES))
def test_a_float32_run_decides_few_pixels_differently(host_frames, case, back):
    """the pose change, and the change back with the tighter thresholds the device test gives its third frame"""
    (g_prev, t_prev, cam_prev), (g, tri, cam), sk, m_prev, m_cur = host_frames[case]
    geo = {}
    if back:
        g_prev, cam_prev, g, tri, m_prev, m_cur = g, cam, g_prev, t_prev, m_cur, m_prev
        geo = dict(normal_cos_min=0.95, plane_tolerance=0.004)
    posed = PC.posed_objects(sk, m_cur)
    objects = {o: (PM.REPOSED, p, m_prev[PC.SKIN_OF[o]]) for o, p in posed.items()}
    records = PM.carry_back(g, tri, objects)
    obj = g.view(np.uint32)[..., 7]
    assert all(np.all(PM.record_states(records)[obj == o] == PM.REPOSED) for o in PC.POSED)
    assert np.all(PM.record_states(records)[~np.isin(obj, PC.POSED)] == PM.UNPOSED)
    hist = np.ones((PC.H, PC.W, 4))
    taps64 = PM.reproject(g, records, hist, g_prev, cam_prev, PC.H, 0, dtype=np.float64, **geo)[2]
    taps32 = PM.reproject(g, records, hist, g_prev, cam_prev, PC.H, 0, dtype=np.float32, **geo)[2]
    differ = int(np.sum(taps64 != taps32))
    kept = {o: round(float(np.mean(taps64[obj == o] >= 0)), 3) for o in PC.POSED}
    print(f"{case}{' back' if back else ''}: {differ} of {PC.W * PC.H} pixels ({differ / (PC.W * PC.H):.4%}) decided differently in float32; "
          f"posed objects keeping history: {kept}; pixels: { {o: int((obj == o).sum()) for o in PC.POSED} }")
    assert all((obj == o).sum() > 40 for o in PC.POSED)                        # every posed object is on the screen
    assert all(k > 0.5 for k in kept.values())                                 # more than half of each keeps its history
    assert differ / (PC.W * PC.H) <= PC.CAP
