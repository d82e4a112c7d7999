"""The numpy statement of CGPT_TEMPORAL_FOLLOW_TRANSFORMS (motion_ref.py) against closed forms, and how many pixels a float32 run of
the statement decides differently on the scene and the moves of the device tests (motion_cases.py).  No GPU."""
import numpy as np
import pytest

import denoise_ref as D
import motion_cases as MC
import motion_ref as M
import temporal_ref as T
from test_temporal_reference import PH, PW, frame, plane_camera, plane_guides, random_acc

IDENTITY = np.eye(3, 4, dtype=np.float32)


def shifted(dx, dy=0.0, dz=0.0):
    m = IDENTITY.copy()
    m[:, 3] = (dx, dy, dz)
    return m


def card_guides(cx, card_x):
    """plane_guides (the wall z = 0, one pixel per world unit, from the camera at (cx, 0, 8)) with a card lying on it: object 1 over
    world x in [card_x - 2, card_x + 2), object 0 elsewhere.  Returns (guides, the card's pixels)."""
    g = plane_guides(cx)
    on = (g[..., 0] >= card_x - 2.0) & (g[..., 0] < card_x + 2.0)
    g.view(np.uint32)[on, 7] = 1
    return g, on


def card_frame(model, acc, n, g, cam, xform, follow=True):
    return frame(model, acc, n, g, cam, xform=xform, follow=follow)


def test_an_object_shifted_by_whole_pixels_takes_its_history_shifted_and_the_background_its_own():
    rng = np.random.default_rng(21)
    cam = plane_camera()
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    g1, on1 = card_guides(0.0, -1.0)                                           # the card over columns 5..8
    g2, on2 = card_guides(0.0, 2.0)                                            # moved three world units = three pixels to the right
    m = M.Temporal()
    out1, _ = card_frame(m, a1, 4, g1, cam, [IDENTITY, shifted(0.0)])
    out2, _ = card_frame(m, a2, 1, g2, cam, [IDENTITY, shifted(3.0)])
    c2 = D.radiance(a2, 1).astype(np.float64)
    cols1, cols2 = np.flatnonzero(on1[0]), np.flatnonzero(on2[0])
    assert list(cols2 - cols1) == [3] * 4
    H = m.history[..., 3]
    assert np.all(H[:, cols2] == 5)                                            # the card: its history, three columns to the left
    assert np.allclose(out2[:, cols2, :3], (4 * out1[:, cols1, :3] + c2[:, cols2]) / 5, rtol=1e-12, atol=0)
    never = ~on1[0] & ~on2[0]                                                  # the wall the card never covered: its own history
    assert np.all(H[:, never] == 5)
    assert np.allclose(out2[:, never, :3], (4 * out1[:, never, :3] + c2[:, never]) / 5, rtol=1e-12, atol=0)
    revealed = on1[0] & ~on2[0]                                                # the wall the card uncovered: H' = N and c_0's bits
    assert revealed.sum() == 3
    assert np.all(H[:, revealed] == 1) and np.array_equal(out2[:, revealed, :3], c2[:, revealed])
    # without the flag the edit drops everything
    m = M.Temporal()
    card_frame(m, a1, 4, g1, cam, [IDENTITY, shifted(0.0)])
    out, _ = card_frame(m, a2, 1, g2, cam, [IDENTITY, shifted(3.0)], follow=False)
    assert np.all(m.history[..., 3] == 1) and np.array_equal(out[..., :3], c2)


def test_an_object_moving_with_the_camera_maps_to_itself_while_the_background_shifts():
    rng = np.random.default_rng(22)
    a1, a2 = random_acc(rng, 4), random_acc(rng, 1)
    g1, on1 = card_guides(0.0, 0.0)
    g2, on2 = card_guides(2.0, 2.0)                                            # camera and card both two units to the right
    assert np.array_equal(on1, on2)
    m = M.Temporal()
    out1, _ = card_frame(m, a1, 4, g1, plane_camera(0.0), [IDENTITY, shifted(0.0)])
    out2, _ = card_frame(m, a2, 1, g2, plane_camera(2.0), [IDENTITY, shifted(2.0)])
    c2 = D.radiance(a2, 1).astype(np.float64)
    cols = np.flatnonzero(on1[0])
    H = m.history[..., 3]
    assert np.all(H[:, cols] == 5)
    assert np.allclose(out2[:, cols, :3], (4 * out1[:, cols, :3] + c2[:, cols]) / 5, rtol=1e-12, atol=0)
    wall = np.flatnonzero(~on2[0])
    kept = [q for q in wall if q + 2 < PW and not on1[0, q + 2]]               # the wall shifts by two columns; behind the old card: none
    assert len(kept) >= 6
    for q in kept:
        assert np.all(H[:, q] == 5)
        assert np.allclose(out2[:, q, :3], (4 * out1[:, q + 2, :3] + c2[:, q]) / 5, rtol=1e-12, atol=0)
    lost = [q for q in wall if q not in kept]
    assert lost and np.all(H[:, lost] == 1)


def test_unmoved_records_are_temporal_ref_bit_for_bit():
    rng = np.random.default_rng(23)
    hist = np.concatenate([rng.uniform(size=(PH, PW, 3)), np.full((PH, PW, 1), 7.0)], -1)
    gp, cam_p = plane_guides(0.0, obj_edge=1.5), plane_camera(0.0)
    g = plane_guides(2.5, obj_edge=1.5)
    mats = np.stack([shifted(0.3, 0.1), MC.affine(MC.rot(1, 30.0), (1, 2, 3))])
    records = M.motion_records(mats, mats)
    assert np.all(M.record_states(records) == M.UNMOVED)
    gc, dropped = M.carry_back(g, records)
    assert np.array_equal(gc.view(np.uint32), g.view(np.uint32)) and not dropped.any()
    for a, b in zip(M.reproject(g, records, hist, gp, cam_p, PH, 0), T.reproject(g, hist, gp, cam_p, PH, 0)):
        assert np.array_equal(a, b)
    # and whole frames: T.Temporal's, with the flag set and nothing moved, under the same and under a changed camera
    accs = [random_acc(rng, 2) for _ in range(3)]
    mt, mm = T.Temporal(), M.Temporal()
    for acc, cx in zip(accs, (0.0, 0.0, 2.0)):
        want = frame(mt, acc, 2, plane_guides(cx), plane_camera(cx))
        got = frame(mm, acc, 2, plane_guides(cx), plane_camera(cx), xform=mats, follow=True)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and np.array_equal(mt.history, mm.history)


def test_a_40_degree_turn_keeps_history_with_the_normal_carried_back_and_none_without():
    rng = np.random.default_rng(24)
    hist = np.concatenate([rng.uniform(size=(PH, PW, 3)), np.full((PH, PW, 1), 7.0)], -1)
    # a tilted card through the middle of the screen, turned by 40 degrees about the view axis through its centre
    nrm = np.array([0.7, 0.0, np.sqrt(0.51)])                                  # n . R_z(40) n = 0.49 cos 40 + 0.51 = 0.885 < 0.9
    cam = plane_camera(0.0)
    centre = np.array([0.0, 0.0, 0.0])

    def tilted_guides(roll):
        """the plane through `centre` with the normal R_z(roll) nrm, seen from (0, 0, 8) through the wall's sample points; the card is
        the part of it with object-space |x|, |y| < 3, everything else a miss"""
        n = MC.rot(2, roll) @ nrm
        px, py = np.meshgrid(np.arange(PW), np.arange(PH))
        d = np.stack([(-8.0 + px) / 8.0, (4.0 - py) / 8.0, -np.ones((PH, PW))], -1)
        o = np.array([0.0, 0.0, 8.0])
        t = ((centre - o) @ n) / (d @ n)
        x = o + d * t[..., None]
        local = x @ MC.rot(2, roll)                                            # R_z(-roll) x
        on = (np.abs(local[..., 0]) < 3.0) & (np.abs(local[..., 1]) < 3.0)
        g = np.zeros((PH, PW, 12), np.float32)
        g[..., 3] = 1e34
        gu = g.view(np.uint32)
        gu[..., 7] = gu[..., 11] = D.NO_HIT
        g[on, 0:3] = x[on]
        g[on, 3] = (t * np.linalg.norm(d, axis=-1))[on]
        g[on, 4:7] = n
        gu[on, 7] = 1
        g[on, 8:11] = 0.5
        gu[on, 11] = 1
        return g, on

    prev = np.stack([IDENTITY, IDENTITY])
    cur = np.stack([IDENTITY, MC.affine(MC.rot(2, 40.0), (0, 0, 0))])
    records = M.motion_records(prev, cur)
    assert list(M.record_states(records)) == [M.UNMOVED, M.MOVED]
    (gp, _), (g, on) = tilted_guides(0.0), tilted_guides(40.0)
    assert on.sum() > 25
    assert float(g[on][0, 4:7] @ gp[PH // 2, PW // 2, 4:7]) < 0.9              # the turn alone fails the normal test
    H = M.reproject(g, records, hist, gp, cam, PH, 0)[1]
    print(f"40 degree turn: {float(np.mean(H[on] > 0)):.1%} of the card's pixels keep history")
    assert np.mean(H[on] > 0) > 0.5                                            # most of the card's pixels keep history
    no_normal, _ = M.carry_back(g, records, normals=False)
    assert np.all(T.reproject(no_normal, hist, gp, cam, PH, 0)[1] == 0)        # positions alone: every tap fails n_prev . n >= 0.9
    assert np.all(T.reproject(g, hist, gp, cam, PH, 0)[1] == 0)                # and nothing carried back: none either


def test_a_drop_record_takes_the_history_from_its_object_only():
    hist = np.ones((PH, PW, 4))
    g = plane_guides(0.0, obj_edge=1.5)
    prev = np.stack([IDENTITY, MC.affine(np.eye(3) * 1e30, (0, 0, 0))])
    cur = np.stack([IDENTITY, MC.affine(np.eye(3) * 1e-30, (0, 0, 0))])
    records = M.motion_records(prev, cur)
    assert list(M.record_states(records)) == [M.UNMOVED, M.DROP]
    H = M.reproject(g, records, hist, g, plane_camera(0.5), PH, 0)[1]
    on = g.view(np.uint32)[..., 7] == 1
    assert np.all(H[on] == 0) and np.mean(H[~on] > 0) > 0.8


# ---- a float32 run of the statement on the device tests' scene and moves -----------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_guides():
    """per move: (guides before, camera before, guides after, camera after, matrices before, matrices after), from the oracle's hits
    on the geometry baked at those matrices -- the way test_temporal_reference.py makes its guides"""
    base = MC.base_matrices()
    s = MC.product_scene(base)

    def guides(mats, view):
        o = MC.oracle_scene(mats)
        o.set_camera(view[0], view[1], MC.FOV, MC.W / MC.H)
        cam = MC.camera(s, view)
        ro, rd = o.camera_rays(MC.W, MC.H)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        t, obj, tri, _ = o.intersect_rays(ro, rd)
        # the product's flattened scene names the objects and materials; the normals are the baked triangles' own
        flat = MC.baked_scene(mats)                                             # names the objects and materials; its triangles carry the baked normals
        g = D.guides_from_hits(flat.flatten(), ro, rd, t, obj, tri).reshape(MC.H, MC.W, 12)
        return g, T.camera_array(cam)

    g0, cam0 = guides(base, MC.BASE)
    out = {}
    for name, (move, view) in MC.MOVES.items():
        mats = move(base)
        g1, cam1 = guides(mats, view)
        out[name] = (g0, cam0, g1, cam1, base, mats)
    return out


@pytest.mark.parametrize("back", [False, True])
@pytest.mark.parametrize("move", list(MC.MOVES))
def test_a_float32_run_decides_few_pixels_differently(oracle_guides, move, back):
    """the move, and the move back with the tighter thresholds the device test gives its third frame"""
    g_prev, cam_prev, g, cam, prev, cur = oracle_guides[move]
    geo = {}
    if back:
        g_prev, cam_prev, g, prev, cur = g, cam, g_prev, cur, prev
        geo = dict(normal_cos_min=0.95, plane_tolerance=0.004)
    records = M.motion_records(prev, cur)
    assert all(M.record_states(records)[o] == M.MOVED for o in MC.MOVING)
    assert all(M.record_states(records)[o] == M.UNMOVED for o in (MC.WALL, MC.LAMP, MC.BALL, MC.STATIC))
    hist = np.ones((MC.H, MC.W, 4))
    taps64 = M.reproject(g, records, hist, g_prev, cam_prev, MC.H, 0, dtype=np.float64, **geo)[2]
    taps32 = M.reproject(g, records, hist, g_prev, cam_prev, MC.H, 0, dtype=np.float32, **geo)[2]
    share = float(np.mean(taps64 != taps32))
    obj = g.view(np.uint32)[..., 7]
    kept = {o: round(float(np.mean(taps64[obj == o] >= 0)), 3) for o in MC.MOVING}
    print(f"{move}{' back' if back else ''}: {share:.4%} of the pixels decided differently in float32; moving objects keeping history: {kept}")
    assert all((obj == o).sum() > 40 for o in MC.MOVING)                       # every moving object is on the screen
    assert all(k > 0.5 for k in kept.values())                                 # more than half of each keeps its history
    assert share < MC.CAP
