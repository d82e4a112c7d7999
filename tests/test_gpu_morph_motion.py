"""Following morph-target poses in the temporal stage on the device (CGPT_TEMPORAL_FOLLOW_MORPHS; csrc/device/denoise.hip:
PreparePoses, morph_carry_back): the carry-back records and whole frames against the numpy statement
(morph_motion_ref.py) for both target layouts, the flags and the moments, what each flag keeps and what drops the history or one object,
no side effects, invariance over render paths, uploads, the top-level tree and device groups, the quality it buys on a morphing mesh,
and the example."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import reference_layout_pair, standin_mesh
from test_gpu_denoise import KERNELS, stats_bytes
from test_gpu_motion import interior, obj_of
from test_gpu_pose_motion import variance_guided
from test_gpu_temporal import SEED, assert_close, bits, raw_call, render_frame
import denoise_ref as D
import morph_motion_cases as MCS
import morph_motion_ref as MM
import motion_cases as MC
import motion_ref as M
import pose_motion_ref as PM
import skin_cases as SC
import temporal_ref as T
import variance_ref as V

pytestmark = pytest.mark.gpu

W, H = MCS.W, MCS.H
LIGHTS, VD = MC.light_materials(), MC.view_dependent_materials()
POSES, MORPHS = N.TEMPORAL_FOLLOW_POSES, N.TEMPORAL_FOLLOW_MORPHS
BOTH = dict(poses=True, morphs=True)


class Rig:
    """a renderer with the scene of morph_motion_cases.py uploaded and the case's skins and targets installed (no pose yet)"""

    def __init__(self, case="nudge", device=0, flags=0, instances=True, instanced=None, mats=None, leaf_order=1, top=None, install=True):
        self.case = MCS.Case(case)
        self.s = MCS.product_scene(mats, instances)
        self.r = P.Renderer(device, flags)
        if top is not None:
            self.r.set_top_level(top)
        self.r.upload(self.s, instanced=instanced)
        self.r.set_tuning(morph_leaf_order=leaf_order)
        self.posed = {}
        if install:
            self.install()

    def placements(self, owners):
        """(object, owner) of every object that takes the owner's skin or targets: the second placement too when it is a copy of its own"""
        out = [(o, o) for o in owners]
        return out + [(MCS.INST_B, MCS.INST_A)] if not self.r.instanced and MCS.INST_A in owners else out

    def install(self):
        for o, k in self.placements(MCS.SKINNED):
            bind, j, w, n_joints, _ = self.case.skins[k]
            self.r.set_skin(o, bind, j, w, n_joints)
        for o, k in self.placements(MCS.MORPHED):
            self.r.set_morph_targets(o, self.case.base[k], self.case.deltas[k])
        self.posed = {}

    def pose(self, which):
        """the device calls that take the scene to the pose `which`: a skin_mesh where the matrices changed, a morph_mesh where the weights did"""
        w, m = self.case.poses(which)
        for o, k in self.placements(MCS.SKINNED):
            if self.posed.get(("m", o), b"") != m[k].tobytes():
                self.r.skin_mesh(o, m[k])
                self.posed[("m", o)] = m[k].tobytes()
        for o, k in self.placements(MCS.MORPHED):
            if self.posed.get(("w", o), b"") != w[k].tobytes():
                self.r.morph_mesh(o, w[k])
                self.posed[("w", o)] = w[k].tobytes()

    def cam(self, view):
        return MCS.camera(self.s, view)

    def triangles(self, cam):
        """the first hits' triangle indices as the wavefront pipeline's round-0 launch finds them, 0 on the triangle object"""
        obj, tri, _, _ = self.r.trace_first_hits(W, H, camera=cam)
        return np.where((obj == MCS.TRI) | (obj == 0xFFFFFFFF), 0, tri).astype(np.uint32)

    def close(self):
        self.r.close()
        self.s.close()


def mirror_triangles(case, o, which):
    """the pose of owner o through the host mirrors (the export path)"""
    w, m = case.poses(which)
    rows = case.base[o] if o not in MCS.MORPHED else P.morph_triangles(case.base[o], case.deltas[o], w[o])
    return P.skin_triangles(rows, case.skins[o][1], case.skins[o][2], m[o]) if o in MCS.SKINNED else rows


def statement_records(case, g, tri, mats=None):
    cur = case.objects("cur", mats)
    return PM.carry_back(g, tri, {o: (MM.REPOSED, cur[o], case.history_of(o)) for o in case.reposed})


def left_out_pixels(g, records, m, geo, motion_records=None):
    """the pixels whose accepted tap set a float32 run of the statement decides differently"""
    t64 = PM.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float64, motion_records=motion_records, **geo)[2]
    t32 = PM.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float32, motion_records=motion_records, **geo)[2]
    return t64 != t32


# ---- 1. the carry-back records against the statement --------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf_order", [1, 0])
@pytest.mark.parametrize("name", list(MCS.CASES))
def test_the_carry_back_records_match_the_reference_statement(name, leaf_order):
    """previous_hits() against pose_motion_ref.carry_back evaluated on the device's own guides and on trace_first_hits' triangle indices:
    equal states, x_p within 4 * 2^-24 (|x| + the object's extent), n_p within 1e-6 -- 5.27's bounds, for its reason: the history corners
    are bit-exact float32, the rest is rounded once.  The history corners of the statement are held to what the device wrote under the
    history's pose: a second context that was given refit_mesh(the mirrors' triangles) has the same trees and the same guides bit for
    bit.  Everything that is not re-posed is state 0 with its own x, n bitwise."""
    rig, yard = Rig(name, leaf_order=leaf_order), Rig(name, install=False)
    try:
        r, case = rig.r, rig.case
        cam0, cam1 = rig.cam(MCS.BASE), rig.cam(case.view)
        rig.pose("hist")
        for o in (MCS.STATIC,) + MCS.MORPHED:
            rows = case.triangles(o, "hist")
            assert np.array_equal(bits(rows), bits(mirror_triangles(case, o, "hist"))), o
            yard.r.refit_mesh(o, rows)
            if o != MCS.TRI:
                assert np.array_equal(r.export_bvh(o), yard.r.export_bvh(o)), o
        render_frame(r, cam0, 2, SEED)
        render_frame(yard.r, cam0, 2, SEED)
        assert np.array_equal(bits(r.guides(camera=cam0)), bits(yard.r.guides(camera=cam0)))
        r.denoise_temporal_following(camera=cam0, **BOTH)
        with pytest.raises(P.DeviceError):
            r.previous_hits()                                                  # nothing was re-posed: no records
        if name == "a_b_a":
            rig.pose("between")
        rig.pose("cur")
        render_frame(r, cam1, 1, SEED + 1)
        g, tri = r.guides(camera=cam1), rig.triangles(cam1)
        r.denoise_temporal_following(camera=cam1, **BOTH)
        obj = obj_of(g)
        if not case.reposed:                                                   # A -> B -> A: every object in state 0, no carry-back launch
            with pytest.raises(P.DeviceError):
                r.previous_hits()
            assert np.mean(r.temporal_history()[..., 3][np.isin(obj, MCS.FOLLOWED)] == 3) > 0.5
            return
        got = r.previous_hits()
        want = statement_records(case, g, tri)
        assert np.array_equal(PM.record_states(got), PM.record_states(want))
        assert np.all(got[..., 7] == 0)
        for o in case.reposed:
            on = obj == o
            assert on.sum() > 40 and np.all(PM.record_states(got)[on] == MM.REPOSED), o
            tol = 4.0 * 2.0 ** -24 * (np.abs(want[on][:, 0:3].astype(np.float64)) + case.extent(o))
            err = np.abs(got[on][:, 0:3].astype(np.float64) - want[on][:, 0:3])
            dn = np.abs(got[on][:, 4:7].astype(np.float64) - want[on][:, 4:7]).max()
            print(f"{name} layout {leaf_order} object {o}: {int(on.sum())} pixels, max |dx_p| {err.max():.3e} (tolerance from {tol.min():.3e}), max |dn_p| {dn:.3e}")
            assert np.all(err <= tol), o
            assert dn <= 1e-6, o
        rest = ~np.isin(obj, case.reposed)
        assert np.all(PM.record_states(got)[rest] == MM.UNPOSED)
        assert np.array_equal(bits(got[rest][:, 0:3]), bits(g[rest][:, 0:3])) and np.array_equal(bits(got[rest][:, 4:7]), bits(g[rest][:, 4:7]))
    finally:
        rig.close()
        yard.close()


# ---- 2. frame by frame against the statement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MCS.CASES))
def test_morphed_objects_match_the_reference_statement(name):
    """Frame by frame from the device's own history: the history's pose, the case's pose, and the history's pose again with other
    parameters and iterations = 0 (the FINAL instantiation).  Left out: the pixels whose tap set float32 decides differently, at most CAP."""
    rig = Rig(name)
    try:
        r, case = rig.r, rig.case
        m = MM.Temporal()
        mats = MCS.base_matrices()
        frames = (("hist", MCS.BASE, 2, {}), ("cur", case.view, 1, {}),
                  ("hist", MCS.BASE, 3, dict(max_history=5.0, normal_cos_min=0.95, plane_tolerance=0.004, keep_view_dependent=True, iterations=0)))
        for k, (which, v, n, params) in enumerate(frames):
            cam = rig.cam(v)
            if name == "a_b_a" and k:
                rig.pose("between")
            rig.pose(which)
            render_frame(r, cam, n, SEED + k)
            acc, g, tri = r.accumulator(), r.guides(camera=cam), rig.triangles(cam)
            posed = case.objects(which)
            left_out = np.zeros((H, W), bool)
            if k:
                geo = {q: params[q] for q in ("normal_cos_min", "plane_tolerance") if q in params}
                prev = {o: m.poses[o] for o in case.reposed}
                records = PM.carry_back(g, tri, {o: (MM.REPOSED, posed[o], MM.history_pose(prev[o]) if len(prev[o]) == 4 else PM.matrices_of(prev[o]))
                                                 for o in case.reposed})
                left_out = left_out_pixels(g, records, m, geo)
                print(f"{name} frame {k}: {int(left_out.sum())} of {W * H} pixels left out")
                assert left_out.mean() <= MCS.CAP
                if case.reposed:
                    with pytest.raises(P.DeviceError):                         # between the pose and the next successful call
                        r.temporal_history()
            rgba, px = r.denoise_temporal_following(camera=cam, **BOTH, **params)
            hist = r.temporal_history()
            ref_rgba, _ = m.frame(acc, n, g, cam, tri=tri, posed=posed, xform=mats, follow_poses=True, follow_morphs=True, height=H,
                                  light_materials=LIGHTS, view_dependent_materials=VD, **params)
            keep = ~left_out
            assert_close(hist[keep], m.history[keep], f"history of frame {k}")
            it = params.get("iterations", 5)
            c = hist[..., :3].astype(np.float64)
            out = (D.atrous(c, g, it, 4.0, 0.2, 0.3) if it else c) * D.demodulation(g, LIGHTS)
            assert_close(rgba[..., :3], out, f"output of frame {k}")
            assert np.all(rgba[..., 3] == 1.0)
            if not left_out.any():
                assert_close(rgba[..., :3], ref_rgba[..., :3], f"output of frame {k} against the whole statement")
            if k:
                Hn, obj = hist[..., 3], obj_of(g)
                for o in MCS.FOLLOWED:
                    share = float(np.mean(Hn[obj == o] > n))
                    print(f"{name} frame {k}: object {o}: {share:.1%} of {int((obj == o).sum())} pixels keep history")
                    assert (obj == o).sum() > 40 and share > 0.5
            m.history = hist.astype(np.float64)                                 # the next step starts from the device's history
    finally:
        rig.close()


# ---- 3. the flags -------------------------------------------------------------------------------------------------------------------------

def following(r, cam, flags, **kw):
    """cgpt_denoise_temporal with `flags` as given, through the ABI"""
    p = N.DenoiseParams(kw.get("iterations", 5), N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    t = N.TemporalParams(64.0, 0.9, 0.01, flags)
    rgba = np.empty((r.n_rows, r.width, 4), np.float32)
    px = np.empty((r.n_rows, r.width), np.uint32)
    r._check(r.L.cgpt_denoise_temporal(r._ctx, C.byref(cam), C.byref(p), C.byref(t), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                       px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
    return rgba, px


def test_the_flag_alone_with_a_transform_change_and_unknown_bits():
    """32u alone follows a morph; 4u | 16u | 32u follows a fused pose and a transform change of the same objects in one frame (the hits go
    back through the pose and then through D = M_prev M_cur^-1, two roundings); bits 2, 8, 64 and 31 are refused with nothing written."""
    rig = Rig("fused")
    try:
        r, case = rig.r, rig.case
        mats0 = MCS.base_matrices()
        mats1 = mats0.copy()
        for k, o in enumerate((MCS.INST_B, MCS.SMOOTH, MCS.STATIC)):
            a, b = mats0[o][:, :3].astype(np.float64), mats0[o][:, 3].astype(np.float64)
            mats1[o] = MC.affine(MC.rot(1, 2.0 * (1 if k % 2 == 0 else -1)) @ a, b + np.array([0.08, -0.05, 0.03]))
        m = MM.Temporal()
        all_flags = N.TEMPORAL_FOLLOW_TRANSFORMS | POSES | MORPHS
        for k, (which, mats, v, n) in enumerate((("hist", mats0, MCS.BASE, 2), ("cur", mats1, case.view, 1), ("hist", mats0, MCS.BASE, 2))):
            cam = rig.cam(v)
            rig.pose(which)
            if k:
                r.update_transforms(mats)
            render_frame(r, cam, n, SEED + k)
            acc, g, tri = r.accumulator(), r.guides(camera=cam), rig.triangles(cam)
            posed = case.objects(which, mats)
            left_out = np.zeros((H, W), bool)
            if k:
                records = PM.carry_back(g, tri, {o: (MM.REPOSED, posed[o], MM.history_pose(m.poses[o]) if len(m.poses[o]) == 4 else PM.matrices_of(m.poses[o]))
                                                 for o in case.reposed})
                left_out = left_out_pixels(g, records, m, {}, M.motion_records(m.xform, mats))
                print(f"all three flags frame {k}: {int(left_out.sum())} of {W * H} pixels left out")
                assert left_out.mean() <= MCS.CAP
            following(r, cam, all_flags)
            hist = r.temporal_history()
            m.frame(acc, n, g, cam, tri=tri, posed=posed, xform=mats, follow=True, follow_poses=True, follow_morphs=True, height=H,
                    light_materials=LIGHTS, view_dependent_materials=VD)
            assert_close(hist[~left_out], m.history[~left_out], f"history of frame {k}")
            if k:
                obj = obj_of(g)
                for o in MCS.FOLLOWED:
                    assert np.mean(hist[..., 3][obj == o] > n) > 0.5, o
            m.history = hist.astype(np.float64)
        cam = rig.cam(MCS.BASE)
        before = bits(r.temporal_history()).copy()
        render_frame(r, cam, 2, SEED + 9)
        for unknown in (2, 8, 64, 0x80000020, MORPHS | 8):                     # an unknown bit: refused, nothing changes
            rc, fb, pb = raw_call(r, cam, None, N.TemporalParams(64.0, 0.9, 0.01, unknown))
            assert rc == N.CGPT_ERR_INVALID and np.all(fb == 7) and np.all(pb == 7), unknown
        rc, fb, pb = raw_call(r, cam, None, N.TemporalParams(64.0, 0.9, 0.01, MORPHS), rgba_n=4 * W * H - 4)
        assert rc == N.CGPT_ERR_INVALID and np.all(fb == 7)                     # a wrong rgba size
        assert np.array_equal(bits(r.temporal_history()), before)
    finally:
        rig.close()
    rig = Rig("nudge")                                                         # 32u alone: only weights changed
    try:
        r = rig.r
        cam = rig.cam(MCS.BASE)
        rig.pose("hist")
        render_frame(r, cam, 2, SEED)
        following(r, cam, MORPHS)
        rig.pose("cur")
        render_frame(r, cam, 2, SEED + 1)
        g = r.guides(camera=cam)
        following(r, cam, MORPHS)
        Hn, obj, st = r.temporal_history()[..., 3], obj_of(g), PM.record_states(r.previous_hits())
        for o in rig.case.reposed:
            assert np.all(st[obj == o] == MM.REPOSED) and np.mean(Hn[obj == o] == 4) > 0.5, o
        assert np.all(st[~np.isin(obj, rig.case.reposed)] == MM.UNPOSED) and np.mean(Hn[interior(obj == MCS.WALL)] == 4) > 0.9
    finally:
        rig.close()


def test_the_moments_ride_on_the_carried_back_taps():
    """cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL and 16u | 32u in `temporal`: the colour history and the records are
    cgpt_denoise_temporal's bit for bit and the variance map is var_t of variance_ref's pooled update on the moments reprojected through
    the carried-back taps."""
    rig, plain = Rig("fused"), Rig("fused")
    try:
        r, case = rig.r, rig.case
        cam0, cam1 = rig.cam(MCS.BASE), rig.cam(case.view)
        n0, n1 = 2, 1
        for q in (rig, plain):
            q.pose("hist")
            render_frame(q.r, cam0, n0, SEED)
        g0 = r.guides(camera=cam0)
        l0_prev = V.luminance(D.radiance(r.accumulator(), n0).astype(np.float64) / D.demodulation(g0, LIGHTS))
        variance_guided(r, cam0, POSES | MORPHS, min_history_frames=1)
        plain.r.denoise_temporal_following(camera=cam0, **BOTH)
        hist0 = r.temporal_history().astype(np.float64)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.r.temporal_history()))
        for q in (rig, plain):
            q.pose("cur")
            render_frame(q.r, cam1, n1, SEED + 1)
        g, tri, acc = r.guides(camera=cam1), rig.triangles(cam1), r.accumulator()
        variance_guided(r, cam1, POSES | MORPHS, min_history_frames=1)
        plain.r.denoise_temporal_following(camera=cam1, **BOTH)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.r.temporal_history()))
        assert np.array_equal(bits(r.previous_hits()), bits(plain.r.previous_hits()))
        records = statement_records(case, g, tri)
        m = MM.Temporal()
        m.history, m.guides, m.camera = hist0, g0, T.camera_array(cam0)
        left_out = left_out_pixels(g, records, m, {})
        assert left_out.mean() <= MCS.CAP
        mom0 = np.stack([l0_prev, np.zeros((H, W)), np.full((H, W), float(n0))], -1)        # the first frame's: mu = l0, v = 0, K = N
        mom_h, Hh, _ = PM.reproject(g, records, np.concatenate([mom0, hist0[..., 3:]], -1), g0, cam0, H, 0)
        vd = np.zeros((H, W), bool)
        hit = D.hit_mask(g)
        vd[hit] = np.asarray(VD)[bits(g[..., 11])[hit]]
        Hh = np.where(vd, 0.0, Hh)
        l0 = V.luminance(D.radiance(acc, n1).astype(np.float64) / D.demodulation(g, LIGHTS))
        _, _, _, var_t, _ = V.merge_moments(l0, n1, mom_h[..., 0], mom_h[..., 1], np.where(Hh > 0, mom_h[..., 2], 0.0))
        assert_close(r.variance()[~left_out], var_t[~left_out], "var_t on the carried-back taps")
        assert np.mean(r.variance()[obj_of(g) == MCS.MOVER] > 0) > 0.5          # moments did arrive on the morphed object
    finally:
        rig.close()
        plain.close()


# ---- 4. each flag keeps its own class ------------------------------------------------------------------------------------------------------

def test_each_flag_keeps_its_own_class_and_every_other_edit_drops_the_history():
    rig = Rig("fused")
    try:
        r, case = rig.r, rig.case
        cam = rig.cam(MCS.BASE)
        state = dict(flags=POSES | MORPHS, which=["hist", "cur"])
        rig.pose("hist")

        def frame(seed):
            render_frame(r, cam, 2, seed)
            following(r, cam, state["flags"])
            return r.temporal_history()[..., 3], obj_of(r.guides(camera=cam))

        def morph():                                                           # the weights alone: cgpt_scene_morph_mesh on every object with targets
            state["which"].reverse()
            w, _ = case.poses(state["which"][0])
            for o in MCS.MORPHED:
                r.morph_mesh(o, w[o])

        def skin(objects=MCS.SKINNED):                                         # the matrices alone: cgpt_scene_skin_mesh
            state["which"].reverse()
            _, m = case.poses(state["which"][0])
            for o in objects:
                r.skin_mesh(o, m[o])

        def under(flags, edit, *a):
            edit(*a)
            state["flags"] = flags

        assert np.all(frame(SEED)[0] == 2)
        assert np.all(frame(SEED + 1)[0] == 4)
        under(POSES | MORPHS, morph)                                           # both flags: kept on most of the frame
        with pytest.raises(P.DeviceError) as e:
            r.temporal_history()                                               # ... and no read-back between a morph and the next call
        assert e.value.code == N.CGPT_ERR_INVALID
        assert np.mean(frame(SEED + 2)[0] == 6) > 0.8
        under(POSES, morph)                                                    # a morph with 16u only drops the frame, background included
        assert np.all(frame(SEED + 3)[0] == 2)
        assert np.all(frame(SEED + 4)[0] == 4)
        under(MORPHS, skin)                                                    # a skin pose with 32u only drops the frame
        assert np.all(frame(SEED + 5)[0] == 2)
        assert np.all(frame(SEED + 6)[0] == 4)
        under(POSES, skin, (MCS.INST_A,))                                      # a fused skin pose with 16u only drops that object only, as before
        Hn, obj = frame(SEED + 7)
        fused = np.isin(obj, (MCS.INST_A, MCS.INST_B))
        assert fused.sum() > 80 and np.all(Hn[fused] == 2) and np.mean(Hn[interior(obj == MCS.WALL)] == 6) > 0.9
        assert np.mean(Hn[np.isin(obj, (MCS.MOVER, MCS.SMOOTH, MCS.STATIC))] == 6) > 0.8
        state["flags"] = N.TEMPORAL_FOLLOW_TRANSFORMS | POSES | MORPHS

        def material():
            rig.s.set_material(MC.M_OTHER, P.Material(albedo=(0.3, 0.9, 0.5)))
            r.update_materials(rig.s)

        def refit():
            r.refit_mesh(MCS.MOVER, case.base[MCS.MOVER])

        def upload():
            r.upload(rig.s)
            rig.install()
            rig.pose("hist")

        for k, edit in enumerate((material, refit, upload)):                   # ... drop it under every flag
            frame(SEED + 10 + 3 * k)
            assert np.all(frame(SEED + 11 + 3 * k)[0] >= 4), f"no history before {edit.__name__}"
            edit()
            assert np.all(frame(SEED + 12 + 3 * k)[0] == 2), edit.__name__
    finally:
        rig.close()


# ---- 5. "no pose known" and installations that come and go drop their object only -------------------------------------------------------------

def dropped_alone(r, cam, objects, n, total):
    """the call dropped exactly `objects`: their pixels hold this frame's n samples, the wall `total` (a reprojected length is a
    float32 quotient of the tap sums: within a few roundings of the integer), and the records say so"""
    g = r.guides(camera=cam)
    Hn, obj, st = r.temporal_history()[..., 3], obj_of(g), PM.record_states(r.previous_hits())
    on = np.isin(obj, objects)
    assert on.sum() > 40 and np.all(st[on] == MM.DROP) and np.all(Hn[on] == n)
    assert not np.any(st[~on] == MM.DROP) and np.mean(np.abs(Hn[interior(obj == MCS.WALL)] - total) <= 8 * 2.0 ** -24 * total) > 0.9


def test_state_2_cases_drop_that_objects_pixels_only():
    rig = Rig("fused")
    try:
        r, case = rig.r, rig.case
        cam = rig.cam(MCS.BASE)
        w_hist, w_cur = case.w_hist, case.w_cur
        pair = (MCS.INST_A, MCS.INST_B)

        def frame(seed, n=2):
            render_frame(r, cam, n, seed)
            r.denoise_temporal_following(camera=cam, **BOTH)

        # targets set but never posed: the scene holds the uploaded triangles, which need not be the base
        for o in (MCS.STATIC, MCS.INST_A):
            r.skin_mesh(o, case.m_hist[o])
        for o in (MCS.INST_A, MCS.SMOOTH, MCS.TRI):
            r.morph_mesh(o, w_hist[o])
        frame(SEED)
        r.morph_mesh(MCS.MOVER, w_hist[MCS.MOVER])                             # its first pose: the history knows none
        frame(SEED + 1)
        dropped_alone(r, cam, (MCS.MOVER,), 2, 4)
        r.morph_mesh(MCS.MOVER, w_cur[MCS.MOVER])                              # from a known pose to a known pose: followed
        frame(SEED + 2)
        on = obj_of(r.guides(camera=cam)) == MCS.MOVER
        assert np.all(PM.record_states(r.previous_hits())[on] == MM.REPOSED) and np.mean(r.temporal_history()[..., 3][on] == 4) > 0.5
        # targets replaced: nothing changes before the next pose (the geometry has not moved), that pose drops the object
        r.set_morph_targets(MCS.MOVER, case.base[MCS.MOVER], case.deltas[MCS.MOVER])
        frame(SEED + 3)
        assert np.all(r.temporal_history()[..., 3] >= 4)                        # every object in state 0
        r.morph_mesh(MCS.MOVER, w_hist[MCS.MOVER])
        frame(SEED + 4)
        dropped_alone(r, cam, (MCS.MOVER,), 2, 10)
        # cleared between two calls, after a morph
        r.morph_mesh(MCS.SMOOTH, w_cur[MCS.SMOOTH])
        r.clear_morph_targets(MCS.SMOOTH)
        frame(SEED + 5)
        dropped_alone(r, cam, (MCS.SMOOTH,), 2, 12)
        # a skin installed anew: the next morph is the morph alone, the history's pose went through the old skin
        bind, j, sw, n_joints, _ = case.skins[MCS.INST_A]
        r.set_skin(MCS.INST_A, bind, j, sw, n_joints)
        r.morph_mesh(MCS.INST_A, w_cur[MCS.INST_A])
        frame(SEED + 6)
        dropped_alone(r, cam, pair, 2, 14)
        # a refit through the second placement before the history: no pose known in it, and the next morph drops both placements
        r.refit_mesh(MCS.INST_B, case.base[MCS.INST_A])
        frame(SEED + 7)                                                        # the refit is an edit of the fourth class: a new history
        assert np.all(r.temporal_history()[..., 3] == 2)
        r.morph_mesh(MCS.INST_A, w_hist[MCS.INST_A])
        frame(SEED + 8)
        dropped_alone(r, cam, pair, 2, 4)
    finally:
        rig.close()


def test_targets_installed_posed_and_cleared_between_two_calls_drop_their_object_only():
    """The first call runs in a context that never held targets or a skin (no triangle index exists); then targets are installed,
    posed and cleared again: the second call must not read an index and drops exactly the object the morph wrote."""
    case = MCS.Case("nudge")
    for top in (False, True):
        s = MCS.product_scene()
        r = P.Renderer(0)
        try:
            r.set_top_level(top)
            r.upload(s)
            cam = MCS.camera(s, MCS.BASE)
            render_frame(r, cam, 2, SEED)
            r.denoise_temporal_following(camera=cam, morphs=True)
            r.set_morph_targets(MCS.MOVER, case.base[MCS.MOVER], case.deltas[MCS.MOVER])
            r.morph_mesh(MCS.MOVER, case.w_cur[MCS.MOVER])
            r.clear_morph_targets(MCS.MOVER)
            render_frame(r, cam, 3, SEED + 1)
            r.denoise_temporal_following(camera=cam, morphs=True)
            dropped_alone(r, cam, (MCS.MOVER,), 3, 5)
        finally:
            r.close()
            s.close()


# ---- 6. a set flag with nothing re-posed; no side effects ---------------------------------------------------------------------------------------

def test_a_set_flag_with_nothing_reposed_is_the_call_without_it_bit_for_bit():
    a, b = Rig("nudge"), Rig("nudge")
    never = Rig("nudge", install=False)                                        # a context that never had targets or a skin
    try:
        for q in (a, b):
            q.pose("hist")
        for o in (MCS.STATIC,) + MCS.MORPHED:
            never.r.refit_mesh(o, a.case.triangles(o, "hist"))
        views = (MCS.BASE, MCS.BASE, MC.CAMERA_MOVE, MC.CAMERA_MOVE)           # no history, same camera, reproject, same camera
        for k, v in enumerate(views):
            cam = a.cam(v)
            for q in (a, b, never):
                render_frame(q.r, cam, 2, SEED + k)
            if k == 2:                                                         # there and back again between two calls: nothing was re-posed
                a.pose("cur")
                a.pose("hist")
                render_frame(a.r, cam, 2, SEED + k)
            kw = dict(iterations=0) if k == 3 else {}
            got = a.r.denoise_temporal_following(camera=cam, **BOTH, **kw)
            want = b.r.denoise_temporal(camera=cam, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), k
            assert np.array_equal(bits(a.r.temporal_history()), bits(b.r.temporal_history())), k
            assert np.array_equal(bits(a.r.guides(camera=cam)), bits(never.r.guides(camera=cam))), k   # targets change no guide byte
        assert np.all(a.r.temporal_history()[..., 3] >= 4)                      # A -> B -> A kept the history
        with pytest.raises(P.DeviceError):
            a.r.previous_hits()                                                # and the carry-back kernel never ran
        cam = a.cam(MCS.BASE)
        for q in (a, b):
            render_frame(q.r, cam, 2, SEED + 9)
        got = variance_guided(a.r, cam, POSES | MORPHS)
        want = b.r.denoise_variance_guided(temporal=True, camera=cam)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(a.r.variance()), bits(b.r.variance()))
    finally:
        for q in (a, b, never):
            q.close()


def test_no_side_effects_and_cgpt_denoise_is_unchanged():
    rig = Rig("fused")
    try:
        r = rig.r
        cam = rig.cam(MCS.BASE)
        rig.pose("hist")
        r.render(W, H, 2, seed=SEED, camera=cam, counters=True)
        r.denoise_temporal_following(camera=cam, **BOTH)
        rig.pose("cur")
        r.reset_accumulator()
        r.render(W, H, 3, seed=SEED + 1, camera=cam, counters=True)

        def state():
            return (bits(r.accumulator()).copy(), r.pixels().copy(), stats_bytes(r), bits(r.guides(camera=cam)).copy())

        plain = [bits(a).copy() for a in r.denoise(camera=cam)]
        before = state()
        r.denoise_temporal_following(camera=cam, **BOTH)
        assert np.mean(r.temporal_history()[..., 3] == 5) > 0.5
        r.denoise_temporal_following(camera=cam, iterations=0, **BOTH)
        variance_guided(r, cam, N.TEMPORAL_FOLLOW_TRANSFORMS | POSES | MORPHS)
        for a, b in zip(before, state()):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        again = [bits(a) for a in r.denoise(camera=cam)]
        assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
        assert r.stats().num_accumulated == 3
    finally:
        rig.close()


# ---- 7. invariance ---------------------------------------------------------------------------------------------------------------------------

def two_frames(rig, kernel=P.KERNEL_AUTO):
    r = rig.r
    cam0, cam1 = rig.cam(MCS.BASE), rig.cam(MC.CAMERA_MOVE)
    rig.pose("hist")
    render_frame(r, cam0, 2, SEED, kernel=kernel)
    first = r.denoise_temporal_following(camera=cam0, **BOTH)
    rig.pose("cur")
    render_frame(r, cam1, 2, SEED + 1, kernel=kernel)
    second = r.denoise_temporal_following(camera=cam1, **BOTH)
    return [bits(a).copy() for a in first + second + (r.temporal_history(), r.previous_hits())]


def test_same_bytes_for_every_render_path_upload_tree_layout_and_device_group():
    outs = []
    configs = [dict(kernel=k) for k in KERNELS[:3]]
    configs += [dict(device=[0, 0], flags=N.CTX_GATHER_PEER_COPY), dict(instanced=False), dict(instanced=True), dict(instances=False), dict(top=True),
                dict(leaf_order=0)]
    for cfg in configs:
        kernel = cfg.pop("kernel", P.KERNEL_AUTO)
        rig = Rig("fused", **cfg)
        try:
            assert rig.r.is_group == ("flags" in cfg)
            outs.append(two_frames(rig, kernel))
        finally:
            rig.close()
    Hn = outs[0][4].view(np.float32)[..., 3]
    assert np.mean(Hn == 4) > 0.5 and np.any(outs[0][5][..., 3] == MM.REPOSED)   # the second frame did reproject, through the records
    for k, o in enumerate(outs[1:]):
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b), k + 1


# ---- 8. quality ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bend", [False, True])
def test_following_a_morphing_mesh_at_1spp_is_closer_to_1024spp_than_the_last_frame_denoised_alone(bend):
    """The diffuse layout of the orbit test at 160x120 under a static camera; the stand-in mesh with one target that pushes every corner
    along its normal by its height, the weight growing by 0.06 a frame for six frames of 1 spp, alone and with 5.27's two-joint bend (2
    degrees a frame).  RMSE of the radiance clamped to [0, 1] against a raw 1024-spp render at the last pose, over the mesh's pixels and
    over the whole frame: the followed call must beat cgpt_denoise of the last frame alone on both (DESIGN.md 5.29 records the ratios)."""
    w, h = 160, 120
    v, i = standin_mesh(3)
    _, s = reference_layout_pair(v, i, 1, aspect=w / h)
    cam = s.camera()
    base = P.triangles_from_arrays(v, i)
    j, wt, n_joints, _ = SC.make_case("bend", base)
    centre = base.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    corners = base.reshape(-1, 3, 6)
    height = (corners[..., 1] - corners[..., 1].min()) / (corners[..., 1].max() - corners[..., 1].min())
    target = np.zeros_like(corners)
    target[..., :3] = height[..., None] * corners[..., 3:]
    target = target.reshape(1, -1, 18)

    def matrices(k):
        return np.stack([SC.matrix(), SC.matrix(SC.rotation((1, 0, 0), 2.0 * k), about=centre)])

    def pose(x, k):
        x.morph_mesh(0, np.float32([0.06 * k]))                                # the stand-in is object 0
        if bend:
            x.skin_mesh(0, matrices(k))

    ref, r = P.Renderer(0), P.Renderer(0)
    try:
        for x in (ref, r):
            x.upload(s)
            x.set_morph_targets(0, base, target)
            if bend:
                x.set_skin(0, base, j, wt, n_joints)
        pose(ref, 5)
        ref.render(w, h, 1024, seed=SEED, camera=cam)
        want = np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64)
        for k in range(6):
            pose(r, k)
            render_frame(r, cam, 1, SEED + 1 + k, w, h)
            temporal = r.denoise_temporal_following(camera=cam, **BOTH)[0]
        alone = r.denoise(camera=cam)[0]
        raw = r.accumulator()[..., :3]
        mesh = obj_of(r.guides(camera=cam)) == 0
        assert mesh.sum() > 500

        def rmse(a, sel):
            return float(np.sqrt(np.mean((np.clip(a[..., :3], 0, 1).astype(np.float64) - want)[sel] ** 2)))
        everywhere = np.ones((h, w), bool)
        for name, sel in (("mesh", mesh), ("frame", everywhere)):
            print(f"morphing mesh{' with the bend' if bend else ''} at 1 spp, {name}: RMSE raw {rmse(raw, sel):.4f} denoised alone {rmse(alone, sel):.4f} "
                  f"followed {rmse(temporal, sel):.4f} ratio followed / alone {rmse(temporal, sel) / rmse(alone, sel):.3f}")
        print(f"mean history length: mesh {float(r.temporal_history()[..., 3][mesh].mean()):.2f} frame {float(r.temporal_history()[..., 3].mean()):.2f}")
        assert rmse(temporal, mesh) < rmse(alone, mesh)
        assert rmse(temporal, everywhere) < rmse(alone, everywhere)
    finally:
        ref.close()
        r.close()
        s.close()


# ---- 9. the example --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, tag", [(["--bulge", "0.3"], "bulge"), (["--bulge", "0.3", "--bend", "2"], "bend")])
def test_example_writes_followed_previews(tmp_path, args, tag):
    import os
    import subprocess
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    out = subprocess.run([exe] + args + ["64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for k in range(8):
        for kind in ("raw", "denoised", "temporal"):
            assert os.path.exists(tmp_path / f"{tag}_{k:02d}_{kind}.ppm"), (k, kind)
    first = [(tmp_path / f"{tag}_00_{kind}.ppm").read_bytes() for kind in ("denoised", "temporal")]
    assert first[0] == first[1]                                                # no history yet: the same image
    for k in range(1, 8):                                                      # from then on the history arrives: the temporal frames differ
        frames = [(tmp_path / f"{tag}_{k:02d}_{kind}.ppm").read_bytes() for kind in ("raw", "denoised", "temporal")]
        assert len(set(frames)) == 3 and len(frames[0]) == len(frames[2]), k
