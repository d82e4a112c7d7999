"""Whole renders replayed bounce by bounce through the context's two probes (tests/replay_ref.py).

Test A.  cgpt_intersect_rays and cgpt_shade_samples chained on the host exactly as `megakernel` chains intersect_scene and shade_bounce
give a second statement of a render.  Per lobe level 0..4 (one context raised by edits, as test_gpu_variant_ladder.py does) and 1 and 4 NEE
candidates, the render of every kernel, through the object list and the top-level tree, with and without counters, must equal the replay:
the accumulator as uint32 words, the packed pixels that follow from it, traced_rays, cgpt_get_retrace_unwalked (0 with counters) and
total_energy_received to 1e-12 of itself (the device's atomic order varies: test_gpu_refit.py's rule).  The first view also runs on a band
of rows, on an interleaved band and in CGPT_MODE_COMPARISON, whose right half (px >= W / 2) is the probe's integrator.  There is no
tolerance: the ABI promises that the probe runs the render's own bounce function, and the build has -ffp-contract=off.  Debug views and
BRUTE_FORCE are left out: the probe does not run them.

Test B.  Every step's records of those replays -- the device's own inputs, and the device's results already fetched -- against the float64
model of tests/shade_ref.py under the rule of DESIGN.md 5.18 (test_gpu_shade_step._check, not restated here), one model call per (level,
candidates, view, hit material) so that a grazing GGX sample does not set the diffuse samples' tolerance; at most 2 % of a configuration's
samples may be undecided."""
import copy

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd.distributed import interleaved_rows
import replay_ref as RP
from replay_ref import assert_render_is as _assert_render_is, expected as _expected, render_view as _render
import shade_cases as CASES
import shade_ref as S
import test_gpu_shade_step as STEP

pytestmark = pytest.mark.gpu

W, H = RP.W, RP.H
KERNELS = RP.KERNELS
BAND = (5, 23)                                                                    # neither end on a tile edge
INTERLEAVE = (4, 3, 1)                                                             # bands of 4 rows, every third, starting at the second
MAX_UNDECIDED = 0.02
CONFIGS = [(level, m) for level in RP.LEVELS for m in RP.CANDIDATES]

_state = {}


def _context(level):
    """The one context of this module at `level` (raised edit by edit; the tests run in ascending order), with the model scene at that level."""
    if "r" not in _state:
        sc, names = RP.build_scene()
        ds = sc.device_scene()
        r = P.Renderer(0)
        r.upload(ds)
        _state.update(r=r, sc=sc, ds=ds, ladder=RP.ladder(names), level=0, replays={}, scenes={})
    assert _state["level"] <= level, "the ladder is walked upwards"
    while _state["level"] < level:
        _state["level"] += 1
        model_edit, device_edit = _state["ladder"][_state["level"]]
        model_edit(_state["sc"])
        device_edit(_state["r"])
    assert _state["sc"].lobe_level() == level
    return _state["r"], _state["sc"], _state["ds"]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    if "r" in _state:
        _state["r"].close()
        _state["ds"].close()
    _state.clear()


def _replays(level, m):
    """{view name: (replay, camera, settings)} of a configuration through the context's own probes, computed once."""
    if (level, m) not in _state.get("replays", {}):
        r, sc, ds = _context(level)
        r.set_nee_candidates(m)
        r.set_top_level(False)
        out = {}
        for view in RP.VIEWS:
            cam = RP.view_camera(ds, view)
            st = S.device_settings(RP.view_settings(view))
            rep = RP.replay(r.intersect_rays, r.shade_samples, RP.camera_rays(cam, W, H), W, H, range(H), view["first_sample"], view["n_samples"],
                            RP.SEED, st)
            out[view["name"]] = (rep, cam, st)
        _state["replays"][level, m] = out
        _state["scenes"].setdefault(level, copy.deepcopy(sc))                   # the model's scene at this level, for test B after the context has moved on
    return _state["replays"][level, m]


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,m", CONFIGS)
def test_every_render_is_the_chain_of_its_steps_bit_for_bit(level, m):
    replays = _replays(level, m)
    r, _, _ = _context(level)
    r.set_nee_candidates(m)
    try:
        for view in RP.VIEWS:
            rep, cam, st = replays[view["name"]]
            whole = _expected(rep, view, np.arange(H))
            assert whole["acc"][..., :3].any() and whole["rays"] > 2 * W * H * view["n_samples"] and whole["unwalked"] == rep["unwalked"]
            print(f"level {level} M {m} {view['name']}: {len(rep['steps'])} steps, {sum(s['idx'].size for s in rep['steps'])} samples, rays {whole['rays']}, "
                  f"unwalked {whole['unwalked']}, energy sum {whole['energy']:.6e}")
            for tree in (False, True):
                r.set_top_level(tree)
                for kernel in KERNELS:
                    for counters in (False, True):
                        what = (level, m, view["name"], "kernel", kernel, "tree", tree, "counters", counters)
                        _assert_render_is(_render(r, view, cam, st, kernel, counters), whole, counters, what)
            r.set_top_level(False)
        # the first view on a band, on an interleaved band and in COMPARISON mode
        view = RP.VIEWS[0]
        rep, cam, st = replays[view["name"]]
        comparison = copy.copy(st)
        comparison.render_mode = P.MODE_COMPARISON
        band = _expected(rep, view, np.arange(*BAND))
        rows = interleaved_rows(H, INTERLEAVE[2], INTERLEAVE[1], INTERLEAVE[0])
        assert rows.size and rows[0] == 4 and not np.array_equal(rows, np.arange(rows[0], rows[0] + rows.size))
        dealt = _expected(rep, view, rows)
        whole = _expected(rep, view, np.arange(H))
        for kernel in KERNELS:
            _assert_render_is(_render(r, view, cam, st, kernel, False, rows=BAND), band, False, (level, m, "band", BAND, "kernel", kernel))
            _assert_render_is(_render(r, view, cam, st, kernel, False, interleave=INTERLEAVE), dealt, False, (level, m, "interleave", INTERLEAVE, "kernel", kernel))
            _assert_render_is(_render(r, view, cam, comparison, kernel, False), whole, False, (level, m, "COMPARISON", "kernel", kernel),
                              columns=slice(W // 2, None), count=False)
    finally:
        r.set_top_level(False)


# ---- B ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,m", CONFIGS)
def test_the_float64_model_on_the_samples_a_render_reaches(level, m):
    replays = _replays(level, m)
    sc = _state["scenes"][level]
    n = undecided = ill = 0
    worst = {g: 0.0 for g in S.GROUPS}
    for view in RP.VIEWS:
        rep, _, _ = replays[view["name"]]
        smp = np.concatenate([s["samples"] for s in rep["steps"]])
        dev = np.concatenate([s["results"] for s in rep["steps"]])
        mats = np.array([ob["mat"] for ob in sc.objects] + [-1], np.int64)[np.where(smp["obj"] == S.NO_HIT, len(sc.objects), smp["obj"])]
        assert smp["depth"].max() >= 3 and np.any((smp["depth"] >= 3) & (smp["is_specular"] != 0))
        for mat in np.unique(mats):
            sel = mats == mat
            c = CASES.call(f"replay_level{level}_M{m}_{view['name']}_mat{mat}", copy.deepcopy(sc), RP.view_settings(view), smp[sel], m)
            c["_device_scene"] = None                                          # the mesh light's total_area is in sc already
            STEP._device[c["name"], None] = dev[sel]                           # what STEP._run would hand to STEP._check
            STEP._check(c)
            e = CASES.evaluate(c)
            devn = S.deviation(dev[sel], e["m64"], ~e["m64"]["undecided"])
            for g in S.GROUPS:
                if e["tol"][g] > 0:
                    worst[g] = max(worst[g], devn[g][0] / e["tol"][g])
            n += int(sel.sum()); undecided += int(e["m64"]["undecided"].sum()); ill += int(e["m64"]["ill"].sum())
    share = undecided / n
    print(f"level {level} M {m}: {n} samples, undecided {undecided} = {share:.4f} (ill-conditioned {ill}); largest deviation / tolerance "
          + "  ".join(f"{g} {worst[g]:.3f}" for g in S.GROUPS))
    assert share <= MAX_UNDECIDED, share
