"""Following skinned poses in the temporal stage on the device (CGPT_TEMPORAL_FOLLOW_POSES; csrc/device/denoise.hip: pose_carry_back,
temporal_merge<.., POSE>): the carry-back records and whole frames against the numpy statement (pose_motion_ref.py), the
moments, both flags at once, what keeps and what drops the history, disocclusion, invariance over render paths, device groups and
uploads, no side effects, and the quality it buys on a bending mesh."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import reference_layout_pair, standin_mesh
from test_gpu_denoise import KERNELS, stats_bytes
from test_gpu_motion import interior, obj_of
from test_gpu_temporal import SEED, assert_close, bits, raw_call, render_frame
import denoise_ref as D
import motion_cases as MC
import motion_ref as M
import pose_motion_cases as PC
import pose_motion_ref as PM
import skin_cases as SC
import temporal_ref as T
import variance_ref as V

pytestmark = pytest.mark.gpu

W, H = PC.W, PC.H
LIGHTS, VD = PC.light_materials(), PC.view_dependent_materials()
FOLLOW_BOTH = N.TEMPORAL_FOLLOW_TRANSFORMS | N.TEMPORAL_FOLLOW_POSES


class Rig:
    """a renderer with the scene of pose_motion_cases.py uploaded and its skins installed (no pose yet)"""

    def __init__(self, case="nudge", device=0, flags=0, instances=True, instanced=None, mats=None):
        self.s = PC.product_scene(mats, instances)
        self.r = P.Renderer(device, flags)
        self.r.upload(self.s, instanced=instanced)
        self.sk, self.base, self.after, self.view = PC.case_poses(case)
        self.install()

    def install(self):
        for o, (bind, j, w, n_joints, _) in self.sk.items():
            self.r.set_skin(o, bind, j, w, n_joints)
        if not self.r.instanced:                                               # two copies: the second placement is posed through a skin of its own
            bind, j, w, n_joints, _ = self.sk[PC.INST_A]
            self.r.set_skin(PC.INST_B, bind, j, w, n_joints)

    def pose(self, matrices):
        for o, m in matrices.items():
            self.r.skin_mesh(o, m)
        if not self.r.instanced:
            self.r.skin_mesh(PC.INST_B, matrices[PC.INST_A])

    def cam(self, view):
        return PC.camera(self.s, view)

    def triangles(self, cam):
        """the first hits' triangle indices as the wavefront pipeline's round-0 launch finds them, 0 on the triangle object"""
        obj, tri, _, _ = self.r.trace_first_hits(W, H, camera=cam)
        return np.where((obj == PC.TRI) | (obj == 0xFFFFFFFF), 0, tri).astype(np.uint32)

    def close(self):
        self.r.close()
        self.s.close()


def variance_guided(r, cam, flags, **kw):
    """cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL and `flags` in `temporal`, through the ABI (the keyword set of
    Renderer.denoise_variance_guided is pinned by test_host_variance.py)"""
    p = N.DenoiseParams(5, N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    t = N.TemporalParams(64.0, 0.9, 0.01, flags)
    v = N.VarianceParams(4.0, kw.get("min_history_frames", 4), N.VARIANCE_TEMPORAL)
    rgba = np.empty((r.n_rows, r.width, 4), np.float32)
    px = np.empty((r.n_rows, r.width), np.uint32)
    r._check(r.L.cgpt_denoise_variance_guided(r._ctx, C.byref(cam), C.byref(p), C.byref(t), C.byref(v), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                              px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
    return rgba, px


def statement_records(rig, g, tri, cur, prev, mats=None):
    posed = PC.posed_objects(rig.sk, cur, mats)
    return PM.carry_back(g, tri, {o: (PM.REPOSED, p, prev[PC.SKIN_OF[o]]) for o, p in posed.items()})


def left_out_pixels(g, records, m, geo, motion_records=None):
    """the pixels whose accepted tap set a float32 run of the statement decides differently"""
    t64 = PM.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float64, motion_records=motion_records, **geo)[2]
    t32 = PM.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float32, motion_records=motion_records, **geo)[2]
    return t64 != t32


# ---- 1. the carry-back records against the statement --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(PC.CASES))
def test_the_carry_back_records_match_the_reference_statement(case):
    """previous_hits() against the statement evaluated on the device's own guides and on trace_first_hits' triangle indices: equal
    states, x_p within 4 * 2^-24 (|x| + the object's extent) -- one rounding plus the float inputs' own spacing -- and n_p within 1e-6.
    The history corners of the statement are held to what the device wrote under the history's pose: a second context that was given
    refit_mesh(skin_f32's triangles) has the same trees and the same guides bit for bit."""
    rig = Rig(case)
    yard = Rig(case)
    try:
        r = rig.r
        cam0, cam1 = rig.cam(PC.BASE), rig.cam(rig.view)
        with pytest.raises(P.DeviceError):
            r.previous_hits()                                                  # none yet
        rig.pose(rig.base)
        for o, (bind, j, w, _, _) in rig.sk.items():                           # the history's pose, through the export path
            hist_rows = PM.SK.skin_f32(bind, j, w, rig.base[o])
            assert np.array_equal(bits(hist_rows), bits(P.skin_triangles(bind, j, w, rig.base[o])))
            yard.r.refit_mesh(o, hist_rows)
            if o != PC.TRI:
                assert np.array_equal(r.export_bvh(o), yard.r.export_bvh(o)), o
        render_frame(r, cam0, 2, SEED)
        render_frame(yard.r, cam0, 2, SEED)
        assert np.array_equal(bits(r.guides(camera=cam0)), bits(yard.r.guides(camera=cam0)))
        r.denoise_temporal(camera=cam0, follow_poses=True)
        with pytest.raises(P.DeviceError):
            r.previous_hits()                                                  # nothing was re-posed: no records
        rig.pose(rig.after)
        render_frame(r, cam1, 1, SEED + 1)
        g, tri = r.guides(camera=cam1), rig.triangles(cam1)
        r.denoise_temporal(camera=cam1, follow_poses=True)
        got = r.previous_hits()
        want = statement_records(rig, g, tri, rig.after, rig.base)
        assert np.array_equal(PM.record_states(got), PM.record_states(want))
        obj = obj_of(g)
        assert np.all(got[..., 7] == 0)
        for o in PC.POSED:
            on = obj == o
            assert on.sum() > 40 and np.all(PM.record_states(got)[on] == PM.REPOSED), o
            ext = PC.extent(o, rig.sk, rig.base)
            tol = 4.0 * 2.0 ** -24 * (np.abs(want[on][:, 0:3].astype(np.float64)) + ext)
            err = np.abs(got[on][:, 0:3].astype(np.float64) - want[on][:, 0:3])
            print(f"{case} object {o}: {int(on.sum())} pixels, max |dx_p| {err.max():.3e} (tolerance from {tol.min():.3e}), "
                  f"max |dn_p| {np.abs(got[on][:, 4:7].astype(np.float64) - want[on][:, 4:7]).max():.3e}")
            assert np.all(err <= tol), o
            assert np.all(np.abs(got[on][:, 4:7].astype(np.float64) - want[on][:, 4:7]) <= 1e-6), o
        rest = ~np.isin(obj, PC.POSED)                                         # everything else: state 0 and the pixel's own x, n
        assert np.all(PM.record_states(got)[rest] == PM.UNPOSED)
        assert np.array_equal(bits(got[rest][:, 0:3]), bits(g[rest][:, 0:3])) and np.array_equal(bits(got[rest][:, 4:7]), bits(g[rest][:, 4:7]))
        n = np.empty(8 * W * H + 1, np.float32)
        assert r.L.cgpt_read_previous_hits(r._ctx, n.ctypes.data_as(C.POINTER(C.c_float)), n.size) == N.CGPT_ERR_INVALID   # a wrong size
    finally:
        rig.close()
        yard.close()


# ---- 2. frame by frame against the statement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(PC.CASES))
def test_posed_objects_match_the_reference_statement(case):
    """Frame by frame from the device's own history: the base pose, the case's pose, and the base pose again with other parameters and
    iterations = 0 (the FINAL instantiation).  Left out: the pixels whose tap set float32 decides differently, at most CAP."""
    rig = Rig(case)
    try:
        r = rig.r
        m = PM.Temporal()
        mats = PC.base_matrices()
        frames = ((rig.base, PC.BASE, 2, {}), (rig.after, rig.view, 1, {}),
                  (rig.base, PC.BASE, 3, dict(max_history=5.0, normal_cos_min=0.95, plane_tolerance=0.004, keep_view_dependent=True, iterations=0)))
        prev = None
        for k, (pose, v, n, params) in enumerate(frames):
            cam = rig.cam(v)
            rig.pose(pose)
            render_frame(r, cam, n, SEED + k)
            acc, g, tri = r.accumulator(), r.guides(camera=cam), rig.triangles(cam)
            left_out = np.zeros((H, W), bool)
            if k:
                geo = {q: params[q] for q in ("normal_cos_min", "plane_tolerance") if q in params}
                left_out = left_out_pixels(g, statement_records(rig, g, tri, pose, prev), m, geo)
                print(f"{case} frame {k}: {int(left_out.sum())} of {W * H} pixels left out")
                assert left_out.mean() <= PC.CAP
                with pytest.raises(P.DeviceError):                             # between the pose and the next successful call
                    r.temporal_history()
            rgba, px = r.denoise_temporal(camera=cam, follow_poses=True, **params)
            hist = r.temporal_history()
            ref_rgba, _ = m.frame(acc, n, g, cam, tri=tri, posed=PC.posed_objects(rig.sk, pose), xform=mats, follow_poses=True, height=H,
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
                for o in PC.DIFFUSE_POSED:
                    share = float(np.mean(Hn[obj == o] > n))
                    print(f"{case} frame {k}: object {o}: {share:.1%} of {int((obj == o).sum())} pixels keep history")
                    assert (obj == o).sum() > 40 and share > 0.5
            m.history = hist.astype(np.float64)                                 # the next step starts from the device's history
            prev = pose
    finally:
        rig.close()


# ---- 3. the moments ------------------------------------------------------------------------------------------------------------------------

def test_the_moments_ride_on_the_carried_back_taps():
    """cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL (the MOMENTS and POSE instantiation): the colour history is
    cgpt_denoise_temporal's bit for bit and the variance map is var_t of variance_ref's pooled update on the moments reprojected
    through the carried-back taps."""
    rig, plain = Rig("swing"), Rig("swing")
    try:
        r = rig.r
        cam0, cam1 = rig.cam(PC.BASE), rig.cam(rig.view)
        n0, n1 = 2, 1
        for q in (rig, plain):
            q.pose(q.base)
            render_frame(q.r, cam0, n0, SEED)
        g0 = r.guides(camera=cam0)
        l0_prev = V.luminance(D.radiance(r.accumulator(), n0).astype(np.float64) / D.demodulation(g0, LIGHTS))
        variance_guided(r, cam0, N.TEMPORAL_FOLLOW_POSES, min_history_frames=1)
        plain.r.denoise_temporal(camera=cam0, follow_poses=True)
        hist0 = r.temporal_history().astype(np.float64)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.r.temporal_history()))
        for q in (rig, plain):
            q.pose(q.after)
            render_frame(q.r, cam1, n1, SEED + 1)
        g, tri, acc = r.guides(camera=cam1), rig.triangles(cam1), r.accumulator()
        variance_guided(r, cam1, N.TEMPORAL_FOLLOW_POSES, min_history_frames=1)
        plain.r.denoise_temporal(camera=cam1, follow_poses=True)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.r.temporal_history()))
        assert np.array_equal(bits(r.previous_hits()), bits(plain.r.previous_hits()))
        records = statement_records(rig, g, tri, rig.after, rig.base)
        m = PM.Temporal()
        m.history, m.guides, m.camera = hist0, g0, T.camera_array(cam0)
        left_out = left_out_pixels(g, records, m, {})
        assert left_out.mean() <= PC.CAP
        mom0 = np.stack([l0_prev, np.zeros((H, W)), np.full((H, W), float(n0))], -1)        # the first frame's: mu = l0, v = 0, K = N
        mom_h, Hh, _ = PM.reproject(g, records, np.concatenate([mom0, hist0[..., 3:]], -1), g0, cam0, H, 0)
        vd = np.zeros((H, W), bool)
        hit = D.hit_mask(g)
        vd[hit] = np.asarray(VD)[bits(g[..., 11])[hit]]
        Hh = np.where(vd, 0.0, Hh)
        l0 = V.luminance(D.radiance(acc, n1).astype(np.float64) / D.demodulation(g, LIGHTS))
        _, _, _, var_t, _ = V.merge_moments(l0, n1, mom_h[..., 0], mom_h[..., 1], np.where(Hh > 0, mom_h[..., 2], 0.0))
        keep = ~left_out
        assert_close(r.variance()[keep], var_t[keep], "var_t on the carried-back taps")
        assert np.mean(r.variance()[obj_of(g) == PC.MOVER] > 0) > 0.5          # moments did arrive on the posed object
    finally:
        rig.close()
        plain.close()


# ---- 4. both flags ---------------------------------------------------------------------------------------------------------------------------

def test_a_pose_and_a_transform_change_of_the_same_objects_in_one_frame():
    """Both flags: the hits go back through the pose and then through D = M_prev M_cur^-1, two roundings to float."""
    rig = Rig("nudge")
    try:
        r = rig.r
        mats0 = PC.base_matrices()
        mats1 = mats0.copy()
        for k, o in enumerate((PC.MOVER, PC.INST_B, PC.SMOOTH, PC.STATIC)):
            a, b = mats0[o][:, :3].astype(np.float64), mats0[o][:, 3].astype(np.float64)
            mats1[o] = MC.affine(MC.rot(1, 2.0 * (1 if k % 2 == 0 else -1)) @ a, b + np.array([0.08, -0.05, 0.03]))
        m = PM.Temporal()
        prev = None
        for k, (pose, mats, v, n) in enumerate(((rig.base, mats0, PC.BASE, 2), (rig.after, mats1, rig.view, 1), (rig.base, mats0, PC.BASE, 2))):
            cam = rig.cam(v)
            rig.pose(pose)
            if k:
                r.update_transforms(mats)
            render_frame(r, cam, n, SEED + k)
            acc, g, tri = r.accumulator(), r.guides(camera=cam), rig.triangles(cam)
            left_out = np.zeros((H, W), bool)
            if k:
                left_out = left_out_pixels(g, statement_records(rig, g, tri, pose, prev, mats), m, {}, M.motion_records(m.xform, mats))
                print(f"both flags frame {k}: {int(left_out.sum())} of {W * H} pixels left out")
                assert left_out.mean() <= PC.CAP
            r.denoise_temporal(camera=cam, follow_transforms=True, follow_poses=True)
            hist = r.temporal_history()
            m.frame(acc, n, g, cam, tri=tri, posed=PC.posed_objects(rig.sk, pose, mats), xform=mats, follow=True, follow_poses=True, height=H,
                    light_materials=LIGHTS, view_dependent_materials=VD)
            assert_close(hist[~left_out], m.history[~left_out], f"history of frame {k}")
            if k:
                obj = obj_of(g)
                for o in PC.DIFFUSE_POSED:
                    assert np.mean(hist[..., 3][obj == o] > n) > 0.5, o
            m.history = hist.astype(np.float64)
            prev = pose
    finally:
        rig.close()


# ---- 5. bit-exact equivalences: what keeps and what drops the history -----------------------------------------------------------------------

def test_a_set_flag_with_nothing_reposed_is_the_call_without_it_bit_for_bit():
    a, b = Rig("nudge"), Rig("nudge")
    try:
        for q in (a, b):
            q.pose(q.base)
        views = (PC.BASE, PC.BASE, MC.CAMERA_MOVE, MC.CAMERA_MOVE)             # no history, same camera, reproject, same camera
        for k, v in enumerate(views):
            cam = a.cam(v)
            for q in (a, b):
                render_frame(q.r, cam, 2, SEED + k)
            if k == 2:                                                         # there and back again between two calls: nothing was re-posed
                a.pose(a.after)
                a.pose(a.base)
                render_frame(a.r, cam, 2, SEED + k)
            kw = dict(iterations=0) if k == 3 else {}
            got = a.r.denoise_temporal(camera=cam, follow_poses=True, **kw)
            want = b.r.denoise_temporal(camera=cam, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), k
            assert np.array_equal(bits(a.r.temporal_history()), bits(b.r.temporal_history())), k
        assert np.all(a.r.temporal_history()[..., 3] >= 4)                      # A -> B -> A kept the history
        with pytest.raises(P.DeviceError):
            a.r.previous_hits()                                                # and the carry-back kernel never ran
        cam = a.cam(PC.BASE)
        for q in (a, b):
            render_frame(q.r, cam, 2, SEED + 9)
        got = variance_guided(a.r, cam, N.TEMPORAL_FOLLOW_POSES)
        want = b.r.denoise_variance_guided(temporal=True, camera=cam)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(a.r.variance()), bits(b.r.variance()))
    finally:
        a.close()
        b.close()


def test_each_flag_keeps_its_own_kind_of_edit_and_every_other_edit_drops_the_history():
    rig = Rig("nudge")
    try:
        r = rig.r
        cam = rig.cam(PC.BASE)
        base_m = PC.base_matrices()
        moved_m = base_m.copy()
        moved_m[PC.MOVER][0, 3] += np.float32(0.1)
        state = dict(poses=[rig.base, rig.after], mats=[base_m, moved_m], flags=dict(follow_poses=True), demodulate=True)
        rig.pose(rig.base)

        def frame(seed):
            render_frame(r, cam, 2, seed)
            r.denoise_temporal(camera=cam, demodulate=state["demodulate"], **state["flags"])
            return r.temporal_history()[..., 3]

        def pose():
            state["poses"].reverse()
            rig.pose(state["poses"][0])

        def transform():
            state["mats"].reverse()
            r.update_transforms(state["mats"][0])

        def with_flags(edit, **flags):
            def run():
                edit()
                state["flags"] = flags
            run.__name__ = f"{edit.__name__} under {sorted(flags)}"
            return run

        def material():
            rig.s.set_material(MC.M_OTHER, P.Material(albedo=(0.3, 0.9, 0.5)))
            r.update_materials(rig.s)

        def smooth():
            flags = np.zeros(PC.N_OBJECTS, np.uint32)
            flags[PC.MOVER] = 1
            r.update_smooth_normals(flags)

        def refit():
            r.refit_mesh(PC.STATIC, PM.SK.skin_f32(*rig.sk[PC.STATIC][:3], rig.base[PC.STATIC]))

        def primitive():
            r.update_primitive(PC.BALL, MC.M_OTHER, center=(-9.6, -4.6, 0.0), radius=2.0)

        def upload():
            r.upload(rig.s)
            rig.install()
            rig.pose(state["poses"][0])

        def demodulate_off():
            state["demodulate"] = False

        assert np.all(frame(SEED) == 2)
        assert np.all(frame(SEED + 1) == 4)
        pose()                                                                 # with the flag: kept on most of the frame
        with pytest.raises(P.DeviceError) as e:
            r.temporal_history()                                               # ... and no read-back in between
        assert e.value.code == N.CGPT_ERR_INVALID
        assert np.mean(frame(SEED + 2) == 6) > 0.8
        r.temporal_reset()
        assert np.all(frame(SEED + 3) == 2)
        both = dict(follow_transforms=True, follow_poses=True)
        drops = (with_flags(pose), with_flags(pose, follow_transforms=True), with_flags(transform, follow_poses=True),
                 with_flags(material, **both), smooth, refit, primitive, upload, demodulate_off)
        for k, edit in enumerate(drops):
            assert np.all(frame(SEED + 2 * k + 4) == 4), f"no history before {edit.__name__}"
            edit()
            assert np.all(frame(SEED + 2 * k + 5) == 2), edit.__name__
        assert np.all(frame(SEED + 40) == 4)
        pose()
        transform()                                                            # both kinds of edit under both flags: kept
        assert np.mean(frame(SEED + 41) == 6) > 0.7
        before = bits(r.temporal_history()).copy()
        render_frame(r, cam, 2, SEED + 42)
        for unknown in (2, 8, 16 | 8, 0x80000010):                             # an unknown bit: refused, nothing changes
            rc, fb, pb = raw_call(r, cam, None, N.TemporalParams(64.0, 0.9, 0.01, unknown))
            assert rc == N.CGPT_ERR_INVALID and np.all(fb == 7) and np.all(pb == 7), unknown
        rc, fb, pb = raw_call(r, cam, None, N.TemporalParams(64.0, 0.9, 0.01, N.TEMPORAL_FOLLOW_POSES), rgba_n=4 * W * H - 4)
        assert rc == N.CGPT_ERR_INVALID and np.all(fb == 7)
        assert np.array_equal(bits(r.temporal_history()), before)
        assert np.mean(frame(SEED + 43) == 8) > 0.6
    finally:
        rig.close()


def test_no_pose_known_drops_that_objects_pixels_only():
    """A refit between two calls is a class-O edit; a refit before the history leaves "no pose known" in it, and the next pose drops the
    object's pixels while everything else keeps its history."""
    rig = Rig("nudge")
    try:
        r = rig.r
        cam = rig.cam(PC.BASE)
        rig.pose(rig.base)
        r.refit_mesh(PC.MOVER, PM.SK.skin_f32(*rig.sk[PC.MOVER][:3], rig.base[PC.MOVER]))   # the same triangles, but no pose of the skin
        render_frame(r, cam, 2, SEED)
        r.denoise_temporal(camera=cam, follow_poses=True)
        r.skin_mesh(PC.MOVER, rig.after[PC.MOVER])
        render_frame(r, cam, 2, SEED + 1)
        g = r.guides(camera=cam)
        r.denoise_temporal(camera=cam, follow_poses=True)
        Hn, obj, st = r.temporal_history()[..., 3], obj_of(g), PM.record_states(r.previous_hits())
        assert np.all(st[obj == PC.MOVER] == PM.DROP) and np.all(st[obj != PC.MOVER] == PM.UNPOSED)
        assert np.all(Hn[obj == PC.MOVER] == 2)
        assert np.mean(Hn[interior(obj == PC.WALL)] == 4) > 0.9
        r.skin_mesh(PC.MOVER, rig.base[PC.MOVER])                              # from a known pose to a known pose: followed
        render_frame(r, cam, 2, SEED + 2)
        r.denoise_temporal(camera=cam, follow_poses=True)
        assert np.mean(r.temporal_history()[..., 3][obj_of(r.guides(camera=cam)) == PC.MOVER] == 4) > 0.5
    finally:
        rig.close()


# ---- 6. disocclusion (under an unchanged camera: the call must reproject all the same) ---------------------------------------------------------

def test_pixels_a_pose_uncovers_start_again_and_the_wall_keeps_its_own():
    rig = Rig("nudge")
    try:
        r = rig.r
        cam = rig.cam(PC.BASE)
        n0, n = 4, 3
        rig.pose(rig.base)
        render_frame(r, cam, n0, SEED)
        r.denoise_temporal(iterations=0, demodulate=False, camera=cam, follow_poses=True)
        g_prev, hist0 = r.guides(camera=cam), r.temporal_history().astype(np.float64)
        away = PC.varied(rig.base[PC.MOVER], rig.sk[PC.MOVER][0], 0.0, (2.5, 0.0, 0.0))   # ten pixels to the right (object space is turned 10 degrees about x)
        r.skin_mesh(PC.MOVER, away)
        render_frame(r, cam, n, SEED + 1)
        g = r.guides(camera=cam)
        rgba, px = r.denoise_temporal(iterations=0, demodulate=False, camera=cam, follow_poses=True)
        hist = r.temporal_history()
        plain_rgba, plain_px = r.denoise(iterations=0, demodulate=False, camera=cam)
        c0 = r.accumulator()[..., :3] / np.float32(n)
        obj_prev, obj = obj_of(g_prev), obj_of(g)
        revealed = interior(obj_prev == PC.MOVER) & (obj == PC.WALL)
        print(f"{int(revealed.sum())} pixels uncovered by the pose")
        assert revealed.sum() >= 20
        assert np.all(hist[..., 3][revealed] == n)
        assert np.array_equal(bits(hist[..., :3])[revealed], bits(c0)[revealed])
        assert np.array_equal(bits(rgba)[revealed], bits(plain_rgba)[revealed]) and np.array_equal(px[revealed], plain_px[revealed])
        never = interior((obj_prev == PC.WALL) & (obj == PC.WALL))
        assert never.sum() > 0.3 * W * H
        assert np.all(hist[..., 3][never] == n0 + n)
        own = (n0 * hist0[..., :3] + n * c0.astype(np.float64)) / (n0 + n)
        assert_close(hist[..., :3][never], own[never], "the wall's own history")
        assert np.mean(hist[..., 3][obj == PC.MOVER] == n0 + n) > 0.5          # and the mesh brought its own along
    finally:
        rig.close()


# ---- 7. invariance ---------------------------------------------------------------------------------------------------------------------------

def two_frames(rig, kernel=P.KERNEL_AUTO):
    r = rig.r
    cam0, cam1 = rig.cam(PC.BASE), rig.cam(MC.CAMERA_MOVE)
    rig.pose(rig.base)
    render_frame(r, cam0, 2, SEED, kernel=kernel)
    first = r.denoise_temporal(camera=cam0, follow_poses=True)
    rig.pose(rig.after)
    render_frame(r, cam1, 2, SEED + 1, kernel=kernel)
    second = r.denoise_temporal(camera=cam1, follow_poses=True)
    return [bits(a).copy() for a in first + second + (r.temporal_history(), r.previous_hits())]


def test_same_bytes_for_every_render_path_device_group_and_upload():
    outs = []
    configs = [dict(kernel=k) for k in KERNELS]
    configs += [dict(device=[0, 0, 0], flags=N.CTX_GATHER_PEER_COPY), dict(device=[0], flags=N.CTX_FORCE_COLLECTIVE)]
    configs += [dict(instanced=False), dict(instanced=True), dict(instances=False)]
    for cfg in configs:
        kernel = cfg.pop("kernel", P.KERNEL_AUTO)
        rig = Rig("with_camera", **cfg)
        try:
            assert rig.r.is_group == ("flags" in cfg)
            outs.append(two_frames(rig, kernel))
        finally:
            rig.close()
    Hn = outs[0][4].view(np.float32)[..., 3]
    g_states = outs[0][5][..., 3]
    assert np.mean(Hn == 4) > 0.5 and np.any(g_states == PM.REPOSED)           # the second frame did reproject, through the records
    for k, o in enumerate(outs[1:]):
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b), k + 1


# ---- 8. no side effects ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [False, True])
def test_no_side_effects_and_cgpt_denoise_is_unchanged(group):
    dev, flags = ([0, 0, 0], N.CTX_GATHER_PEER_COPY) if group else (0, 0)
    rig = Rig("swing", dev, flags)
    try:
        r = rig.r
        cam = rig.cam(PC.BASE)
        rig.pose(rig.base)
        r.render(W, H, 2, seed=SEED, camera=cam, counters=True)
        r.denoise_temporal(camera=cam, follow_poses=True)
        rig.pose(rig.after)
        r.reset_accumulator()
        r.render(W, H, 3, seed=SEED + 1, camera=cam, counters=True)

        def state():
            return (bits(r.accumulator()).copy(), r.pixels().copy(), stats_bytes(r), bits(r.guides(camera=cam)).copy())

        plain = [bits(a).copy() for a in r.denoise(camera=cam)]
        before = state()
        r.denoise_temporal(camera=cam, follow_poses=True)
        assert np.mean(r.temporal_history()[..., 3] == 5) > 0.5
        r.denoise_temporal(camera=cam, follow_poses=True, iterations=0)
        variance_guided(r, cam, FOLLOW_BOTH)
        after = state()
        for a, b in zip(before, after):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        again = [bits(a) for a in r.denoise(camera=cam)]
        assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
        assert r.stats().num_accumulated == 3
    finally:
        rig.close()


# ---- 9. quality ------------------------------------------------------------------------------------------------------------------------------------

def test_following_a_bending_mesh_at_1spp_is_closer_to_1024spp_than_the_last_frame_denoised_alone():
    """The diffuse layout of the orbit test at 160x120 under a static camera; the stand-in mesh under the two-joint bend, which grows 2
    degrees a frame for six frames of 1 spp.  RMSE of the radiance clamped to [0, 1] against a raw 1024-spp render at the last pose, over
    the mesh's pixels and over the whole frame: the flagged call must beat cgpt_denoise of the last frame alone on both (DESIGN.md 5.27
    records the measured ratios).  Without the flag every frame's temporal output is its no-history output."""
    w, h = 160, 120
    v, i = standin_mesh(3)
    _, s = reference_layout_pair(v, i, 1, aspect=w / h)
    cam = s.camera()
    bind = P.triangles_from_arrays(v, i)
    j, wt, n_joints, _ = SC.make_case("bend", bind)
    centre = bind.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)

    def matrices(k):
        return np.stack([SC.matrix(), SC.matrix(SC.rotation((1, 0, 0), 2.0 * k), about=centre)])

    ref, r, q = P.Renderer(0), P.Renderer(0), P.Renderer(0)
    try:
        for x in (ref, r, q):
            x.upload(s)
            x.set_skin(0, bind, j, wt, n_joints)                               # the stand-in is object 0
        ref.skin_mesh(0, matrices(5))
        ref.render(w, h, 1024, seed=SEED, camera=cam)
        want = np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64)
        for k in range(6):
            for x in (r, q):
                x.skin_mesh(0, matrices(k))
                render_frame(x, cam, 1, SEED + 1 + k, w, h)
            temporal = r.denoise_temporal(camera=cam, follow_poses=True)[0]
            unflagged = q.denoise_temporal(camera=cam)[0]
            q.temporal_reset()
            assert np.array_equal(bits(unflagged), bits(q.denoise_temporal(camera=cam)[0])), k   # without the flag: no history, every frame
        alone = r.denoise(camera=cam)[0]
        raw = r.accumulator()[..., :3]
        mesh = obj_of(r.guides(camera=cam)) == 0
        assert mesh.sum() > 500

        def rmse(a, sel):
            return float(np.sqrt(np.mean((np.clip(a[..., :3], 0, 1).astype(np.float64) - want)[sel] ** 2)))
        everywhere = np.ones((h, w), bool)
        for name, sel in (("mesh", mesh), ("frame", everywhere)):
            print(f"bending mesh at 1 spp, {name}: RMSE raw {rmse(raw, sel):.4f} denoised alone {rmse(alone, sel):.4f} followed {rmse(temporal, sel):.4f} "
                  f"ratio followed / alone {rmse(temporal, sel) / rmse(alone, sel):.3f}")
        print(f"mean history length: mesh {float(r.temporal_history()[..., 3][mesh].mean()):.2f} frame {float(r.temporal_history()[..., 3].mean()):.2f}")
        assert rmse(temporal, mesh) < rmse(alone, mesh)
        assert rmse(temporal, everywhere) < rmse(alone, everywhere)
    finally:
        for x in (ref, r, q):
            x.close()


# ---- 10. the example -------------------------------------------------------------------------------------------------------------------------------

def test_example_writes_bend_previews(tmp_path):
    import os
    import subprocess
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    out = subprocess.run([exe, "--bend", "3", "64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for k in range(8):
        for kind in ("raw", "denoised", "temporal"):
            assert os.path.exists(tmp_path / f"bend_{k:02d}_{kind}.ppm"), (k, kind)
    first = [(tmp_path / f"bend_00_{kind}.ppm").read_bytes() for kind in ("denoised", "temporal")]
    last = [(tmp_path / f"bend_07_{kind}.ppm").read_bytes() for kind in ("raw", "denoised", "temporal")]
    assert first[0] == first[1]                                                # no history yet: the same image
    assert len(set(last)) == 3 and len(last[0]) == len(last[2])


# ---- 11. skins that come and go between two flagged calls --------------------------------------------------------------------------------------

def test_a_skin_installed_posed_and_cleared_between_two_calls_drops_its_object_only():
    """cgpt_scene_set_skin and cgpt_scene_clear_skin bump no generation.  The first call runs in a context that never held a skin (no
    triangle index exists); then a skin is installed, posed and cleared again: the second call sees no skin, must not read an index, and
    drops exactly the object the pose wrote.  With the top-level tree on and off."""
    sk, base, after, _ = PC.case_poses("swing")
    for top in (False, True):
        s = PC.product_scene()
        r = P.Renderer(0)
        try:
            r.set_top_level(top)
            r.upload(s)
            cam = PC.camera(s, PC.BASE)
            render_frame(r, cam, 2, SEED)
            r.denoise_temporal(camera=cam, follow_poses=True)
            bind, j, w, n_joints, _ = sk[PC.MOVER]
            r.set_skin(PC.MOVER, bind, j, w, n_joints)
            r.skin_mesh(PC.MOVER, after[PC.MOVER])
            r.clear_skin(PC.MOVER)
            render_frame(r, cam, 3, SEED + 1)
            g = r.guides(camera=cam)
            r.denoise_temporal(camera=cam, follow_poses=True)
            Hn, obj, st = r.temporal_history()[..., 3], obj_of(g), PM.record_states(r.previous_hits())
            assert (obj == PC.MOVER).sum() > 40
            assert np.all(st[obj == PC.MOVER] == PM.DROP) and np.all(st[obj != PC.MOVER] == PM.UNPOSED)
            assert np.all(Hn[obj == PC.MOVER] == 3)
            assert np.mean(Hn[interior(obj == PC.WALL)] == 5) > 0.9
        finally:
            r.close()
            s.close()


def test_a_replaced_skin_drops_its_object_after_the_next_pose_and_nothing_before_it():
    rig, plain = Rig("swing"), Rig("swing")
    try:
        r = rig.r
        cam = rig.cam(PC.BASE)
        for q in (rig, plain):
            q.pose(q.base)
            render_frame(q.r, cam, 2, SEED)
            q.r.denoise_temporal(camera=cam, follow_poses=True)
        bind, j, w, n_joints, _ = rig.sk[PC.MOVER]
        r.set_skin(PC.MOVER, bind, j, w, n_joints)                             # another installation; the geometry has not moved
        for q in (rig, plain):
            render_frame(q.r, cam, 2, SEED + 1)
        got, want = r.denoise_temporal(camera=cam, follow_poses=True), plain.r.denoise_temporal(camera=cam)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(r.temporal_history()), bits(plain.r.temporal_history()))
        assert np.all(r.temporal_history()[..., 3] == 4)
        r.skin_mesh(PC.MOVER, rig.after[PC.MOVER])                             # the history knows the old installation's pose: no way back
        render_frame(r, cam, 2, SEED + 2)
        g = r.guides(camera=cam)
        r.denoise_temporal(camera=cam, follow_poses=True)
        Hn, obj, st = r.temporal_history()[..., 3], obj_of(g), PM.record_states(r.previous_hits())
        assert np.all(st[obj == PC.MOVER] == PM.DROP) and np.all(st[obj != PC.MOVER] == PM.UNPOSED)
        assert np.all(Hn[obj == PC.MOVER] == 2) and np.mean(Hn[interior(obj == PC.WALL)] == 6) > 0.9
        r.skin_mesh(PC.MOVER, rig.base[PC.MOVER])                              # from now on both sides know this installation
        render_frame(r, cam, 2, SEED + 3)
        r.denoise_temporal(camera=cam, follow_poses=True)
        on = obj_of(r.guides(camera=cam)) == PC.MOVER
        assert np.all(PM.record_states(r.previous_hits())[on] == PM.REPOSED) and np.mean(r.temporal_history()[..., 3][on] == 4) > 0.5
    finally:
        rig.close()
        plain.close()
