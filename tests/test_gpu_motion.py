"""Following object transforms in the temporal stage on the device (CGPT_TEMPORAL_FOLLOW_TRANSFORMS; csrc/device/denoise.hip:
temporal_merge<.., MOTION>): moved objects against the numpy statement (motion_ref.py), disocclusion, the view-dependent
rule, a set flag with nothing moved, what drops the history, invariance over render paths, device groups, uploads and bands, no side
effects, the quality it buys on a turning mesh, and the example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import reference_layout_pair, standin_mesh
from test_gpu_denoise import KERNELS, stats_bytes
from test_gpu_temporal import SEED, assert_close, bits, raw_call, render_frame
import denoise_ref as D
import motion_cases as MC
import motion_ref as M
import temporal_ref as T
import variance_ref as V

pytestmark = pytest.mark.gpu

W, H = MC.W, MC.H
LIGHTS, VD = MC.light_materials(), MC.view_dependent_materials()
DIFFUSE_MOVERS = (MC.MOVER, MC.INST_A, MC.INST_B)


def new_renderer(mats=None, device=0, flags=0, instances=True, instanced=None):
    s = MC.product_scene(mats, instances)
    r = P.Renderer(device, flags)
    r.upload(s, instanced=instanced)
    return s, r


def variance_guided_following(r, cam, **kw):
    """cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL and CGPT_TEMPORAL_FOLLOW_TRANSFORMS in `temporal`, through the ABI: the
    keyword set of Renderer.denoise_variance_guided is pinned by test_host_variance.py, so the binding passes the flag on denoise_temporal only"""
    p = N.DenoiseParams(5, N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    t = N.TemporalParams(64.0, 0.9, 0.01, N.TEMPORAL_FOLLOW_TRANSFORMS)
    v = N.VarianceParams(4.0, kw.get("min_history_frames", 4), N.VARIANCE_TEMPORAL)
    rgba = np.empty((r.n_rows, r.width, 4), np.float32)
    px = np.empty((r.n_rows, r.width), np.uint32)
    r._check(r.L.cgpt_denoise_variance_guided(r._ctx, C.byref(cam), C.byref(p), C.byref(t), C.byref(v), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                              px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
    return rgba, px


def obj_of(g):
    return bits(g[..., 7])


def left_out_pixels(g, records, m, geo):
    """the pixels whose accepted tap set a float32 run of the statement decides differently"""
    t64 = M.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float64, **geo)[2]
    t32 = M.reproject(g, records, m.history, m.guides, m.camera, H, 0, dtype=np.float32, **geo)[2]
    return t64 != t32


def interior(mask):
    """the pixels whose 3x3 neighbourhood lies in the mask"""
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out &= np.roll(np.roll(mask, dy, 0), dx, 1)
    out[0], out[-1], out[:, 0], out[:, -1] = False, False, False, False
    return out


# ---- 1. against the statement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", list(MC.MOVES))
def test_moved_objects_match_the_reference_statement(move):
    """Frame by frame from the device's own history: the base frame, the move, and the move back with other parameters and
    iterations = 0 (the FINAL instantiation).  Left out: the pixels whose tap set float32 decides differently, at most CAP."""
    base = MC.base_matrices()
    change, view = MC.MOVES[move]
    s, r = new_renderer(base)
    try:
        m = M.Temporal()
        frames = ((base, MC.BASE, 2, {}), (change(base), view, 1, {}),
                  (base, MC.BASE, 3, dict(max_history=5.0, normal_cos_min=0.95, plane_tolerance=0.004, keep_view_dependent=True, iterations=0)))
        for k, (mats, v, n, params) in enumerate(frames):
            cam = MC.camera(s, v)
            if k:
                r.update_transforms(mats)
            render_frame(r, cam, n, SEED + k)
            acc, g = r.accumulator(), r.guides(camera=cam)
            left_out = np.zeros((H, W), bool)
            if k:
                records = M.motion_records(m.xform, mats)
                geo = {q: params[q] for q in ("normal_cos_min", "plane_tolerance") if q in params}
                left_out = left_out_pixels(g, records, m, geo)
                print(f"{move} frame {k}: {int(left_out.sum())} of {W * H} pixels left out")
                assert left_out.mean() <= MC.CAP
                with pytest.raises(P.DeviceError):                             # between the edit and the next successful call
                    r.temporal_history()
            rgba, px = r.denoise_temporal(camera=cam, follow_transforms=True, **params)
            hist = r.temporal_history()
            ref_rgba, _ = m.frame(acc, n, g, cam, xform=mats, follow=True, height=H, light_materials=LIGHTS, view_dependent_materials=VD, **params)
            keep = ~left_out
            assert_close(hist[keep], m.history[keep], f"history of frame {k}")
            it = params.get("iterations", 5)
            c = hist[..., :3].astype(np.float64)
            out = (D.atrous(c, g, it, 4.0, 0.2, 0.3) if it else c) * D.demodulation(g, LIGHTS)
            assert_close(rgba[..., :3], out, f"output of frame {k}")
            assert np.all(rgba[..., 3] == 1.0)
            assert np.max(np.abs(((px[..., None] >> np.uint32([0, 8, 16])) & 0xFF).astype(int) -
                                 ((D.pack_pixels(out)[..., None] >> np.uint32([0, 8, 16])) & 0xFF).astype(int))) <= 1
            if not left_out.any():
                assert_close(rgba[..., :3], ref_rgba[..., :3], f"output of frame {k} against the whole statement")
            if k:
                Hn, obj = hist[..., 3], obj_of(g)
                for o in DIFFUSE_MOVERS + ((MC.GLASS,) if params.get("keep_view_dependent") else ()):
                    share = float(np.mean(Hn[obj == o] > n))
                    print(f"{move} frame {k}: object {o}: {share:.1%} of {int((obj == o).sum())} pixels keep history")
                    assert (obj == o).sum() > 40 and share > 0.5
            m.history = hist.astype(np.float64)                                 # the next step starts from the device's history
    finally:
        r.close()


@pytest.mark.parametrize("move", list(MC.MOVES))
def test_the_moments_ride_on_the_carried_back_taps(move):
    """cgpt_denoise_variance_guided with CGPT_VARIANCE_TEMPORAL (the MOMENTS instantiation): the colour history is cgpt_denoise_temporal's
    and the variance map is var_t of variance_ref's pooled update on the moments reprojected through the carried-back taps."""
    base = MC.base_matrices()
    change, view = MC.MOVES[move]
    mats = change(base)
    s, r = new_renderer(base)
    s2, plain = new_renderer(base)
    try:
        cam0, cam1 = MC.camera(s, MC.BASE), MC.camera(s, view)
        n0, n1 = 2, 1
        for q in (r, plain):
            render_frame(q, cam0, n0, SEED)
        g0 = r.guides(camera=cam0)
        mod0 = D.demodulation(g0, LIGHTS)
        l0_prev = V.luminance(D.radiance(r.accumulator(), n0).astype(np.float64) / mod0)
        variance_guided_following(r, cam0, min_history_frames=1)
        plain.denoise_temporal(camera=cam0, follow_transforms=True)
        hist0 = r.temporal_history().astype(np.float64)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.temporal_history()))
        for q in (r, plain):
            q.update_transforms(mats)
            render_frame(q, cam1, n1, SEED + 1)
        g = r.guides(camera=cam1)
        acc = r.accumulator()
        variance_guided_following(r, cam1, min_history_frames=1)
        plain.denoise_temporal(camera=cam1, follow_transforms=True)
        assert np.array_equal(bits(r.temporal_history()), bits(plain.temporal_history()))
        records = M.motion_records(base, mats)
        m = M.Temporal()
        m.history, m.guides, m.camera = hist0, g0, T.camera_array(cam0)
        left_out = left_out_pixels(g, records, m, {})
        assert left_out.mean() <= MC.CAP
        mom0 = np.stack([l0_prev, np.zeros((H, W)), np.full((H, W), float(n0))], -1)        # the first frame's: mu = l0, v = 0, K = N
        mom_h, Hh, _ = M.reproject(g, records, np.concatenate([mom0, hist0[..., 3:]], -1), g0, cam0, H, 0)
        vd = np.zeros((H, W), bool)
        hit = D.hit_mask(g)
        vd[hit] = np.asarray(VD)[bits(g[..., 11])[hit]]
        Hh = np.where(vd, 0.0, Hh)
        l0 = V.luminance(D.radiance(acc, n1).astype(np.float64) / D.demodulation(g, LIGHTS))
        _, _, _, var_t, _ = V.merge_moments(l0, n1, mom_h[..., 0], mom_h[..., 1], np.where(Hh > 0, mom_h[..., 2], 0.0))
        keep = ~left_out
        assert_close(r.variance()[keep], var_t[keep], "var_t on the carried-back taps")
        obj = obj_of(g)
        assert np.mean(r.variance()[obj == MC.MOVER] > 0) > 0.5                # moments did arrive on the moved object
    finally:
        r.close()
        plain.close()


# ---- 2. disocclusion, 3. the view-dependent rule (both under an unchanged camera: the call must reproject all the same) ---------------

def test_pixels_the_object_uncovered_start_again_and_the_background_keeps_its_own():
    base = MC.base_matrices()
    s, r = new_renderer(base)
    try:
        cam = MC.camera(s, MC.BASE)
        n0, n = 4, 3
        render_frame(r, cam, n0, SEED)
        r.denoise_temporal(iterations=0, demodulate=False, camera=cam, follow_transforms=True)
        g_prev, hist0 = r.guides(camera=cam), r.temporal_history().astype(np.float64)
        mats = base.copy()
        mats[MC.MOVER][0, 3] += np.float32(2.5)                                # ten pixels to the right, parallel to the screen
        r.update_transforms(mats)
        render_frame(r, cam, n, SEED + 1)
        g = r.guides(camera=cam)
        rgba, px = r.denoise_temporal(iterations=0, demodulate=False, camera=cam, follow_transforms=True)
        hist = r.temporal_history()
        plain_rgba, plain_px = r.denoise(iterations=0, demodulate=False, camera=cam)
        c0 = r.accumulator()[..., :3] / np.float32(n)
        obj_prev, obj = obj_of(g_prev), obj_of(g)
        revealed = interior(obj_prev == MC.MOVER) & (obj != MC.MOVER)
        print(f"{int(revealed.sum())} pixels uncovered by the object")
        assert revealed.sum() >= 20
        assert np.all(hist[..., 3][revealed] == n)
        assert np.array_equal(bits(hist[..., :3])[revealed], bits(c0)[revealed])
        assert np.array_equal(bits(rgba)[revealed], bits(plain_rgba)[revealed]) and np.array_equal(px[revealed], plain_px[revealed])
        never = interior((obj_prev == MC.WALL) & (obj == MC.WALL))             # the wall it never covered: its own history
        assert never.sum() > 0.4 * W * H
        assert np.all(hist[..., 3][never] == n0 + n)
        own = (n0 * hist0[..., :3] + n * c0.astype(np.float64)) / (n0 + n)
        assert_close(hist[..., :3][never], own[never], "the background's own history")
        on = obj == MC.MOVER                                                   # and the object brought its own along
        assert np.mean(hist[..., 3][on] == n0 + n) > 0.5
    finally:
        r.close()


def test_glass_restarts_after_its_move_and_keeps_its_history_with_the_flag():
    base = MC.base_matrices()
    mats = MC.MOVES["turn"][0](base)
    s, r = new_renderer(base)
    try:
        cam = MC.camera(s, MC.BASE)

        def second_frame(**kw):
            r.temporal_reset()
            r.update_transforms(base)
            render_frame(r, cam, 2, SEED)
            r.denoise_temporal(iterations=0, camera=cam, follow_transforms=True)
            r.update_transforms(mats)
            render_frame(r, cam, 2, SEED + 1)
            r.denoise_temporal(iterations=0, camera=cam, follow_transforms=True, **kw)
            glass = obj_of(r.guides(camera=cam)) == MC.GLASS
            assert glass.sum() > 100
            return r.temporal_history()[..., 3], glass

        Hn, glass = second_frame()
        assert np.all(Hn[glass] == 2)                                          # the camera bytes are equal, but the call reprojects
        assert np.mean(Hn[~glass] == 4) > 0.8
        Hn, glass = second_frame(keep_view_dependent=True)
        assert np.mean(Hn[glass] > 2) > 0.5
    finally:
        r.close()


# ---- 4. nothing moved ------------------------------------------------------------------------------------------------------------------

def test_a_set_flag_with_nothing_moved_is_the_call_without_it_bit_for_bit():
    base = MC.base_matrices()
    s, a = new_renderer(base)
    s2, b = new_renderer(base)
    try:
        views = (MC.BASE, MC.BASE, MC.CAMERA_MOVE, MC.CAMERA_MOVE)             # no history, same camera, reproject, same camera
        for k, v in enumerate(views):
            cam = MC.camera(s, v)
            for q in (a, b):
                render_frame(q, cam, 2, SEED + k)
            if k in (1, 2):
                a.update_transforms(base)                                      # an edit that moves nothing: kept with the flag
                render_frame(a, cam, 2, SEED + k)
            kw = dict(iterations=0) if k == 3 else {}
            got = a.denoise_temporal(camera=cam, follow_transforms=True, **kw)
            want = b.denoise_temporal(camera=cam, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), k
            assert np.array_equal(bits(a.temporal_history()), bits(b.temporal_history())), k
        assert np.all(a.temporal_history()[..., 3] >= 4)                        # the history did survive the edits
        for q in (a, b):                                                       # the variance-guided call too
            render_frame(q, MC.camera(s, MC.BASE), 2, SEED + 9)
        got = variance_guided_following(a, MC.camera(s, MC.BASE))
        want = b.denoise_variance_guided(temporal=True, camera=MC.camera(s, MC.BASE))
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(a.variance()), bits(b.variance()))
    finally:
        a.close()
        b.close()


# ---- 5. what drops the history ----------------------------------------------------------------------------------------------------------

def test_a_clear_flag_and_every_other_edit_drop_the_history_and_a_refused_call_does_not():
    base = MC.base_matrices()
    moved = MC.MOVES["shift"][0](base)
    s, r = new_renderer(base)
    try:
        cam = MC.camera(s, MC.BASE)
        size = [W, H]
        state = dict(demodulate=True, follow=True, mats=[base, moved])

        def frame(seed):
            render_frame(r, cam, 2, seed, size[0], size[1])
            r.denoise_temporal(camera=cam, demodulate=state["demodulate"], follow_transforms=state["follow"])
            return r.temporal_history()[..., 3]

        def transform():
            state["mats"].reverse()
            r.update_transforms(state["mats"][0])

        def transform_flag_clear():
            transform()
            state["follow"] = False

        def material():
            state["follow"] = True
            s.set_material(MC.M_OTHER, P.Material(albedo=(0.3, 0.9, 0.5)))
            r.update_materials(s)

        def smooth():
            flags = np.zeros(MC.N_OBJECTS, np.uint32)
            flags[MC.MOVER] = 1
            r.update_smooth_normals(flags)

        def refit():
            v, i = MC.meshes()[1]
            w = v.copy()
            w[:, :3] *= np.float32(0.9)
            r.refit_mesh(MC.MOVER, P.triangles_from_arrays(w, i))

        def refit_through_an_instance():
            v, i = MC.meshes()[2]
            w = v.copy()
            w[:, 1] *= np.float32(0.8)
            r.refit_mesh(MC.INST_B, P.triangles_from_arrays(w, i))

        def primitive():
            r.update_primitive(MC.BALL, MC.M_OTHER, center=(-9.6, -4.6, 0.0), radius=2.0)

        def smaller():
            size[1] = H - 3

        def demodulate_off():
            state["demodulate"] = False

        assert np.all(frame(SEED) == 2)
        assert np.all(frame(SEED + 1) == 4)
        transform()                                                            # with the flag: kept on most of the frame
        with pytest.raises(P.DeviceError) as e:
            r.temporal_history()                                               # ... and no read-back in between
        assert e.value.code == N.CGPT_ERR_INVALID
        assert np.mean(frame(SEED + 2) == 6) > 0.8
        r.temporal_reset()
        assert np.all(frame(SEED + 3) == 2)
        for k, edit in enumerate((transform_flag_clear, material, smooth, refit, refit_through_an_instance, primitive, smaller, demodulate_off)):
            assert np.all(frame(SEED + 2 * k + 4) == 4), f"no history before {edit.__name__}"
            edit()
            assert np.all(frame(SEED + 2 * k + 5) == 2), edit.__name__
        assert np.all(frame(SEED + 30) == 4)
        before = bits(r.temporal_history()).copy()
        render_frame(r, cam, 2, SEED + 31, size[0], size[1])
        for unknown in (2, 8, 4 | 8, 0x80000004):                              # an unknown bit: refused, nothing changes
            rc, fb, pb = raw_call(r, cam, None, N.TemporalParams(64.0, 0.9, 0.01, unknown))
            assert rc == N.CGPT_ERR_INVALID and np.all(fb == 7) and np.all(pb == 7), unknown
        assert np.array_equal(bits(r.temporal_history()), before)
        assert np.all(frame(SEED + 32) == 6)
        transform()
        transform()                                                            # there and back again: the bytes are equal, nothing moved
        assert np.all(frame(SEED + 33) == 8)
    finally:
        r.close()


# ---- 6. invariance ------------------------------------------------------------------------------------------------------------------------

def two_frames(s, r, kernel=P.KERNEL_AUTO, rows=None):
    base = MC.base_matrices()
    change, view = MC.MOVES["with_camera"]
    kw = {} if rows is None else dict(rows=rows)
    cam0, cam1 = MC.camera(s, MC.BASE), MC.camera(s, view)
    render_frame(r, cam0, 2, SEED, kernel=kernel, **kw)
    first = r.denoise_temporal(camera=cam0, follow_transforms=True)
    r.update_transforms(change(base))
    render_frame(r, cam1, 2, SEED + 1, kernel=kernel, **kw)
    second = r.denoise_temporal(camera=cam1, follow_transforms=True)
    return [bits(a).copy() for a in first + second + (r.temporal_history(),)]


def test_same_bytes_for_every_render_path_device_group_and_upload():
    outs = []
    configs = [dict(kernel=k) for k in KERNELS]
    configs += [dict(device=[0, 0, 0], flags=N.CTX_GATHER_PEER_COPY), dict(device=[0], flags=N.CTX_FORCE_COLLECTIVE)]
    configs += [dict(instanced=False), dict(instanced=True), dict(instances=False)]
    for cfg in configs:
        kernel = cfg.pop("kernel", P.KERNEL_AUTO)
        s, r = new_renderer(MC.base_matrices(), **cfg)
        try:
            assert r.is_group == ("flags" in cfg)
            outs.append(two_frames(s, r, kernel))
        finally:
            r.close()
    Hn = outs[0][4].view(np.float32)[..., 3]
    assert np.mean(Hn == 4) > 0.5                                              # the second frame did reproject
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)


def test_a_contiguous_band_reprojects_with_its_global_rows():
    rows = (10, 47)
    base = MC.base_matrices()
    change, view = MC.MOVES["with_camera"]
    s, r = new_renderer(base)
    try:
        m = M.Temporal()
        for k, (mats, v) in enumerate(((base, MC.BASE), (change(base), view))):
            cam = MC.camera(s, v)
            if k:
                r.update_transforms(mats)
            render_frame(r, cam, 2, SEED + k, rows=rows)
            g = r.guides(camera=cam)
            assert g.shape == (37, W, 12)
            left_out = np.zeros(g.shape[:2], bool)
            if k:
                rec = M.motion_records(base, mats)
                t64 = M.reproject(g, rec, m.history, m.guides, m.camera, H, rows[0], dtype=np.float64)[2]
                t32 = M.reproject(g, rec, m.history, m.guides, m.camera, H, rows[0], dtype=np.float32)[2]
                left_out = t64 != t32
                assert left_out.mean() <= MC.CAP
            rgba, _ = r.denoise_temporal(camera=cam, follow_transforms=True)
            m.frame(r.accumulator(), 2, g, cam, xform=mats, follow=True, height=H, first_row=rows[0], light_materials=LIGHTS, view_dependent_materials=VD)
            assert_close(r.temporal_history()[~left_out], m.history[~left_out], f"band history {k}")
        obj = obj_of(g)
        assert np.mean(m.history[..., 3][obj == MC.MOVER] == 4) > 0.5
    finally:
        r.close()


# ---- 7. no side effects ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [False, True])
def test_no_side_effects_and_cgpt_denoise_is_unchanged(group):
    base = MC.base_matrices()
    dev, flags = ([0, 0, 0], N.CTX_GATHER_PEER_COPY) if group else (0, 0)
    s, r = new_renderer(base, dev, flags)
    try:
        cam = MC.camera(s, MC.BASE)
        r.render(W, H, 2, seed=SEED, camera=cam, counters=True)
        r.denoise_temporal(camera=cam, follow_transforms=True)
        r.update_transforms(MC.MOVES["turn"][0](base))
        r.reset_accumulator()
        r.render(W, H, 3, seed=SEED + 1, camera=cam, counters=True)

        def state():
            return (bits(r.accumulator()).copy(), r.pixels().copy(), stats_bytes(r), bits(r.guides(camera=cam)).copy())

        plain = [bits(a).copy() for a in r.denoise(camera=cam)]
        before = state()
        r.denoise_temporal(camera=cam, follow_transforms=True)
        assert np.mean(r.temporal_history()[..., 3] == 5) > 0.5
        r.denoise_temporal(camera=cam, follow_transforms=True, iterations=0)
        variance_guided_following(r, cam)
        after = state()
        for a, b in zip(before, after):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        again = [bits(a) for a in r.denoise(camera=cam)]
        assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
        assert r.stats().num_accumulated == 3
    finally:
        r.close()


# ---- 8. quality -------------------------------------------------------------------------------------------------------------------------------

def spun(centre, deg):
    """the matrix of a turn by `deg` about the vertical axis through `centre`"""
    a = MC.rot(1, deg)
    return MC.affine(a, np.asarray(centre, np.float64) - a @ np.asarray(centre, np.float64))


def test_following_a_turning_mesh_at_1spp_is_closer_to_1024spp_than_the_last_frame_denoised_alone():
    """The diffuse layout of the orbit test at 160x120 under a static camera; the stand-in mesh turns 2 degrees a frame for six frames
    of 1 spp.  RMSE of the radiance clamped to [0, 1] against a raw 1024-spp render at the last pose, over the mesh's pixels and over the
    whole frame: the flagged call must beat cgpt_denoise of the last frame alone on both (DESIGN.md 5.25 records the measured ratios).
    Without the flag every frame's temporal output is its no-history output."""
    w, h = 160, 120
    v, i = standin_mesh(3)
    _, s = reference_layout_pair(v, i, 1, aspect=w / h)
    cam = s.camera()
    n_obj = s.flatten().n_objects
    centre = 0.5 * (v[:, :3].min(0) + v[:, :3].max(0)).astype(np.float64)

    def matrices(k):
        m = np.tile(np.eye(3, 4, dtype=np.float32), (n_obj, 1, 1))
        m[0] = spun(centre, 2.0 * k)                                           # the stand-in is object 0
        return m

    ref, r, q = P.Renderer(0), P.Renderer(0), P.Renderer(0)
    try:
        for x in (ref, r, q):
            x.upload(s)
        ref.update_transforms(matrices(5))
        ref.render(w, h, 1024, seed=SEED, camera=cam)
        want = np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64)
        for k in range(6):
            for x in (r, q):
                x.update_transforms(matrices(k))
                render_frame(x, cam, 1, SEED + 1 + k, w, h)
            temporal = r.denoise_temporal(camera=cam, follow_transforms=True)[0]
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
            print(f"turning mesh at 1 spp, {name}: RMSE raw {rmse(raw, sel):.4f} denoised alone {rmse(alone, sel):.4f} followed {rmse(temporal, sel):.4f} "
                  f"ratio followed / alone {rmse(temporal, sel) / rmse(alone, sel):.3f}")
        print(f"mean history length: mesh {float(r.temporal_history()[..., 3][mesh].mean()):.2f} frame {float(r.temporal_history()[..., 3].mean()):.2f}")
        assert rmse(temporal, mesh) < rmse(alone, mesh)
        assert rmse(temporal, everywhere) < rmse(alone, everywhere)
    finally:
        for x in (ref, r, q):
            x.close()


# ---- 9. the example ---------------------------------------------------------------------------------------------------------------------------

def test_example_writes_spin_previews(tmp_path):
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    out = subprocess.run([exe, "--spin", "3", "64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for k in range(8):
        for kind in ("raw", "denoised", "temporal"):
            assert os.path.exists(tmp_path / f"spin_{k:02d}_{kind}.ppm"), (k, kind)
    first = [(tmp_path / f"spin_00_{kind}.ppm").read_bytes() for kind in ("denoised", "temporal")]
    last = [(tmp_path / f"spin_07_{kind}.ppm").read_bytes() for kind in ("raw", "denoised", "temporal")]
    assert first[0] == first[1]                                                # no history yet: the same image
    assert len(set(last)) == 3 and len(last[0]) == len(last[2])
