"""cgpt_set_stream: every entry point on a caller-provided stream.

The yardstick is a twin context that never leaves its own stream and is driven with the same calls; every comparison is to the bit.
Equality alone cannot tell which stream ran a kernel, so part 2 queues a delay and a copy into the accumulator on the caller's stream
and then calls the library: the call must see the copied data, which the twin is given through the host path (load_accumulator).  A
launch, copy or event site that used the context's own stream would read the accumulator before the copy lands.  Part 3 pins that torch's
default stream, whose handle is 0 on ROCm and which the C ABI would read as "the context's own stream", is refused under each of its
names.  Part 4 switches streams in the middle of an accumulation, shares one stream between two contexts, and pins
the refusals; part 5 reads the framebuffer through the device pointers.

The delay (part 2).  A chain of 2048^2 float32 matmuls on resident tensors, its length set from a calibration on the same stream to
max(5 x the twin's wall time for the same call on its own stream, 20 ms), at most 250 ms.  Each case asserts that the stream is still
busy when the library is called -- a case whose delay ran out fails, it never passes for nothing -- and prints the chain's device time
(torch events) beside the call's wall time.  Measured on an MI355X, (delay ms, call ms) per case, 0.123 ms a link:
    megakernel (19.6, 0.52), persistent_two_streams (19.5, 2.16), wavefront (19.6, 1.35), denoise (19.5, 0.07),
    accumulator (19.5, 0.01), reset_accumulator (19.4, 0.05)
-- the 20 ms floor decides every case; it is nine times the slowest call.

What part 2 can and cannot see (measured).  A build whose denoise_prepare launch uses the own stream fails the denoise
case and the denoiser's equality test.  A build whose wavefront pool streams do not wait for the caller's stream still passes all of
it: while the chain runs, a megakernel or pipeline render of this library on ANY other stream -- its own included -- ends only when
the chain does (17 ms against 0.5-1.3 ms alone, whichever of eight streams holds the chain), though a denoise (0.46 ms), a reset
(0.14 ms), a persistent-kernel render (8 ms) and a one-kernel torch op (0.05 ms) on another stream finish beside it, unless the two
streams share a hardware queue (they do every fourth).  So the denoise, reset and persistent cases see a wrong stream run early; a
megakernel or pipeline launch on the wrong stream runs when the chain ends, racing the queued copy, and is caught when it loses that
race or breaks the order inside its own call, not for certain.  Each case runs on four consecutive streams so that a shared hardware
queue, which orders two streams by itself, hides a missing wait on one of them at most.
The two-stream case of the persistent kernel renders 1024 x 512: that kernel forks onto its pool streams only when a call has more
than one batch, the smallest batch limit is 1 Mi paths (pt_max_paths_mi = 1), and three samples of 512 Ki pixels are the smallest call
that crosses it.  Every other frame is 64 x 48 or 64 x 64."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.distributed import _DevicePointer
import shade_cases as SC
import shade_ref as SR
import trace_cases as TC
import test_gpu_morph as MORPH
import test_gpu_pose_batch as BATCH
import test_gpu_skinning as SKIN
from test_gpu_morph import assert_same_scene
from test_gpu_pose_batch import RECIPE, eased, entries_of, one_by_one
from test_gpu_refit import BIG, SUN, WALL, assert_same_frames, frames, fresh, random_rays
from test_gpu_skinning import KERNELS, MESHES, OCTA, SIZE, STRIP256, bits, build_scene
from test_host_binned_build import soup_mesh

pytestmark = pytest.mark.gpu

W, H = 64, 48
SEED = 0x2468ACE1
STATS = ("traced_rays", "inner_steps", "tri_tests", "bvh_depth_sum", "closest_hits", "num_accumulated")
THREE_KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT)


def same(got, ref, what=""):
    """tuples of arrays, byte for byte"""
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: output {k}: {np.count_nonzero(a.view(np.uint8) != b.view(np.uint8))} bytes differ"


def counters(ctx):
    st = ctx.stats()
    return tuple(getattr(st, c) for c in STATS)


def on_stream(scene, stream):
    """a context put on `stream` before its scene is uploaded"""
    r = P.Renderer(0)
    r.set_stream(stream)
    r.upload(scene)
    return r


@pytest.fixture(scope="module")
def world():
    s, binds = build_scene()
    yield s, binds
    s.close()


LANES = 4


@pytest.fixture(scope="module")
def lanes():
    """Caller's streams made one after another, none the default stream or a blocking one.  Part 2 runs on each: streams that share a
    hardware queue are ordered by the hardware, so a pool stream that does not wait for the caller's stream still runs behind it when
    the two share one, and the case passes for nothing.  A process opens four hardware queues unless GPU_MAX_HW_QUEUES says otherwise,
    and the runtime deals new streams over them: of four consecutive streams at most one shares the queue of a given pool stream."""
    streams = [torch.cuda.Stream() for _ in range(LANES)]
    assert len({s.cuda_stream for s in streams} | {0}) == LANES + 1
    return streams


@pytest.fixture(scope="module")
def side(lanes):
    """S: the caller's stream of the parts that need one"""
    return lanes[0]


@pytest.fixture()
def pair(world, side):
    s, binds = world
    r, want = on_stream(s, side), fresh(s)
    yield s, binds, r, want
    r.close(); want.close()


# ---- 1. every entry point on a caller's stream equals the own stream ------------------------------------------------------------
@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_COMPARISON])
@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT, P.KERNEL_AUTO])
def test_renders_and_the_framebuffer(pair, kernel, mode):
    s, _, r, want = pair
    st = P.Settings(render_mode=mode)
    for ctx in (r, want):
        ctx.reset_accumulator(); ctx.reset_stats()
        ctx.render(W, H, 3, seed=SEED, kernel=kernel, counters=True, settings=st)
    acc = want.accumulator()
    same((r.accumulator(), r.pixels()), (acc, want.pixels()), "first render")
    assert counters(r) == counters(want) and r.stats().num_accumulated == 3
    assert r.stats().kernel_ms > 0                                            # the timing events were recorded on the caller's stream
    for ctx in (r, want):                                                     # a checkpoint through the host, then the accumulation goes on
        ctx.reset_accumulator()
        ctx.load_accumulator(acc, 3, W, H)
        same((ctx.accumulator(),), (acc,), "load_accumulator")
        ctx.render(W, H, 2, seed=SEED, kernel=kernel, counters=True, settings=st)
    same((r.accumulator(), r.pixels()), (want.accumulator(), want.pixels()), "continued render")
    assert counters(r) == counters(want) and r.num_accumulated == 5 and r.stats().num_accumulated == 5
    assert not np.array_equal(bits(r.accumulator()), bits(acc))


def test_the_trace_probes(side):
    _, s = TC.parity_pair(2)
    r, want = on_stream(s, side), fresh(s)
    o, d = (a[:4096] for a in TC.parity_rays())
    so, sd, st = TC.nee_shadow_rays(2)
    try:
        same(r.intersect_rays(o, d), want.intersect_rays(o, d), "intersect_rays")
        tm = np.where(np.arange(o.shape[0]) % 2 == 0, np.float32(4.0), TC.T_FAR).astype(np.float32)
        same(r.intersect_rays(o, d, tm), want.intersect_rays(o, d, tm), "intersect_rays with tmax")
        for count in (False, True):
            for reverse in (False, True):
                for ctx in (r, want):
                    ctx.reset_stats()
                same(r.trace_rays(o, d, None, so, sd, st, counters=count, reverse=reverse),
                     want.trace_rays(o, d, None, so, sd, st, counters=count, reverse=reverse), ("trace_rays", count, reverse))
                assert counters(r) == counters(want)
            same(r.trace_first_hits(W, H, counters=count), want.trace_first_hits(W, H, counters=count), ("trace_first_hits", count))
            same(r.trace_first_hits(45, 37, rows=(5, 30), counters=count), want.trace_first_hits(45, 37, rows=(5, 30), counters=count), "a band")
        assert (r.trace_rays(o, d)[1] != TC.NO_HIT).sum() > 1000              # the rays do hit something
    finally:
        r.close(); want.close()


def test_the_shade_probe(side):
    c = SC.calls_of("state_rules")[0]                                         # the smallest batch of tests/shade_cases.py
    s = c["scene"].device_scene()
    r, want = on_stream(s, side), fresh(s)
    try:
        st = SR.device_settings(c["settings"])
        got, ref = r.shade_samples(c["samples"], st), want.shade_samples(c["samples"], st)
        same((got,), (ref,), "shade_samples")
        assert c["samples"].shape[0] > 16 and ref.view(np.uint8).any()
    finally:
        r.close(); want.close(); s.close()


def checked(r, want, k):
    """the exported trees, a ray batch and one frame; the kernel and the walk take turns from edit to edit"""
    assert_same_scene(r, want, configs=KERNELS[k % 4:k % 4 + 1], tops=(bool(k & 1),))


def test_scene_edits_of_materials_transforms_and_geometry(side):
    s, binds = build_scene()                                                  # a scene of its own: its materials are edited
    r, want = on_stream(s, side), fresh(s)
    both = (r, want)
    try:
        n_mat, n_obj = s.flatten().n_materials, s.flatten().n_objects
        before = frames(want, sizes=SIZE, configs=KERNELS[:1])
        s.set_material(0, P.Material(albedo=(0.9, 0.3, 0.2), specular=0.4, roughness=0.3))
        for ctx in both:
            ctx.update_materials(s)
        checked(r, want, 0)
        assert not np.array_equal(frames(want, sizes=SIZE, configs=KERNELS[:1])[0][0], before[0][0])
        rough = np.linspace(0.1, 0.6, n_mat).astype(np.float32)
        for ctx in both:
            ctx.update_roughness(rough)
        checked(r, want, 1)
        for ctx in both:
            ctx.update_transmission_roughness(rough[::-1])
        checked(r, want, 2)
        smooth = np.zeros(n_obj, np.uint32); smooth[[BIG, SKIN.TRI, SKIN.STRIP257]] = 1
        for ctx in both:
            ctx.update_smooth_normals(smooth)
        checked(r, want, 3)
        m = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (n_obj, 1))
        m[BIG] = np.float32([[0.8, 0, 0.6, 0.4], [0, 1, 0, -0.2], [-0.6, 0, 0.8, 0.3]]).ravel()
        m[STRIP256] = np.float32([[1, 0, 0, 0.5], [0, 1.5, 0, 0], [0, 0, 1, 0.2]]).ravel()
        for ctx in both:
            ctx.update_transforms(m)
        checked(r, want, 4)
        for ctx in both:
            ctx.update_primitive(SUN, 2, center=(-6.0, 9.0, 4.0), radius=3.5)
            ctx.update_primitive(WALL, 1, normal=(0.0, 0.6, 0.8), point=(0.0, 0.0, -12.0))
        checked(r, want, 5)
        moved = binds[BIG].copy().reshape(-1, 3, 6); moved[..., :3] += np.float32([0.3, 0.1, -0.4])
        areas = [ctx.refit_mesh(BIG, moved.reshape(-1, 18)) for ctx in both]
        assert bits(np.float32(areas[0])) == bits(np.float32(areas[1]))
        checked(r, want, 6)
        assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    finally:
        r.close(); want.close(); s.close()


def test_scene_edits_of_skins_morph_targets_and_batches(pair):
    s, binds, r, want = pair
    both = (r, want)
    skins = [SKIN.install(ctx, binds, "bend") for ctx in both][0]
    checked(r, want, 0)                                                       # set_skin alone moves nothing
    assert np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    for ctx in both:
        for obj, (j, w, m) in skins.items():
            ctx.skin_mesh(obj, m)
    checked(r, want, 1)
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    morphs = [MORPH.install(ctx, binds, "mix") for ctx in both][0]
    checked(r, want, 2)
    for ctx in both:
        for obj, (base, d, w) in morphs.items():
            ctx.morph_mesh(obj, w)                                            # fused with the posed skins
    checked(r, want, 3)
    for ctx in both:
        for obj in SKIN.SKINNED:
            ctx.clear_skin(obj)
    checked(r, want, 4)
    for ctx in both:
        for obj in MORPH.MORPHED:
            ctx.clear_morph_targets(obj)
    checked(r, want, 5)
    with pytest.raises(P.DeviceError, match="has no skin"):
        r.skin_mesh(BIG, skins[BIG][2])
    cases = [BATCH.install(ctx, binds) for ctx in both][0]                    # the RECIPE mix: skin only, morph only and both
    assert cases.keys() == RECIPE.keys()
    tree = r.export_bvh(OCTA)
    r.pose_objects(entries_of(cases)); one_by_one(want, entries_of(cases))    # the twin by the single calls
    checked(r, want, 6)
    assert not np.array_equal(r.export_bvh(OCTA), tree)
    again = entries_of(eased(cases, 0.5))
    r.pose_objects(again); want.pose_objects(again)
    checked(r, want, 7)
    for top in (True, False):                                                 # the tree over the objects is written on the stream too
        for ctx in both:
            ctx.set_top_level(top)
        o, d = random_rays(4096, 5)
        same(r.intersect_rays(o, d), want.intersect_rays(o, d), ("top level", top))
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))


def denoiser_outputs(ctx, call):
    rgba, px = call()
    return rgba, px, ctx.guides()


def test_the_denoiser(pair):
    s, binds, r, want = pair
    both = (r, want)
    cases = [BATCH.install(ctx, binds) for ctx in both][0]
    for ctx in both:
        ctx.pose_objects(entries_of(cases))
        ctx.reset_accumulator(); ctx.render(W, H, 2, seed=SEED)
    same(denoiser_outputs(r, lambda: r.denoise(iterations=2)), denoiser_outputs(want, lambda: want.denoise(iterations=2)), "denoise")
    same(denoiser_outputs(r, lambda: r.denoise_variance_guided(iterations=2)), denoiser_outputs(want, lambda: want.denoise_variance_guided(iterations=2)),
         "denoise_variance_guided")
    same((r.variance(),), (want.variance(),), "variance")
    follow = dict(iterations=1, poses=True, morphs=True)
    for frame, ease in enumerate((None, 0.4)):                                # two frames with a batch between them: the second reprojects
        for ctx in both:
            if ease is not None:
                ctx.pose_objects(entries_of(eased(cases, ease)))
            ctx.reset_accumulator(); ctx.render(W, H, 2, seed=SEED + frame)
        same(denoiser_outputs(r, lambda: r.denoise_temporal_following(**follow)), denoiser_outputs(want, lambda: want.denoise_temporal_following(**follow)),
             ("denoise_temporal_following", frame))
        same((r.temporal_history(),), (want.temporal_history(),), ("temporal_history", frame))
    same((r.previous_hits(),), (want.previous_hits(),), "previous_hits")
    assert np.any(want.temporal_history()[..., 3] > 2)                        # the history was used
    assert np.any(bits(want.previous_hits())[..., 3] == 1)                    # and hits were carried back


@pytest.mark.parametrize("option", [P.BUILD_NAIVE, P.BUILD_SAH_INTERVALS, P.BUILD_SAH_PRIMITIVES, P.BUILD_SAH_BINNED])
def test_build_bvh(side, option):
    mesh = soup_mesh(6, 257)
    s = P.Scene()
    s.add_material(P.Material())
    s.add_mesh(mesh, 0, P.BUILD_SAH_INTERVALS)
    desc = s.flatten()
    obj = desc.objects[0]
    ptr = C.cast(C.addressof(desc.triangles.contents) + obj.tri_offset * C.sizeof(N.Triangle), C.POINTER(N.Triangle))
    r, want = P.Renderer(0), P.Renderer(0)
    r.set_stream(side)
    try:
        got, ref = r.build_bvh(ptr, obj.tri_count, option), want.build_bvh(ptr, obj.tri_count, option)
        same(got[:2], ref[:2], "nodes and triangle order")
        assert got[2] == ref[2] and bits(np.float32(got[3])) == bits(np.float32(ref[3])) and obj.tri_count == 257
        assert sorted(got[1].tolist()) == list(range(257))
    finally:
        r.close(); want.close(); s.close()


def test_measure_issue_rate(side):
    r = P.Renderer(0)
    r.set_stream(side)
    try:
        rate, ms = r.measure_issue_rate(iters=2000)
        assert rate > 0 and ms > 0
    finally:
        r.close()


# ---- 2. a call waits for what the caller queued in front of it --------------------------------------------------------------------
class Delay:
    """A chain of device-side matmuls on resident tensors, calibrated on the stream it will be queued on."""
    N = 2048

    def __init__(self, stream):
        with torch.cuda.stream(stream):
            self.a = torch.full((self.N, self.N), 1.0 / self.N, device="cuda:0")
            self.b, self.c = self.a.clone(), torch.empty_like(self.a)
            self.queue_links(8)                                               # the BLAS handle and workspace of this stream
            stream.synchronize()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(); self.queue_links(32); end.record()
            end.synchronize()
            self.ms_per_link = start.elapsed_time(end) / 32
        assert self.ms_per_link > 0

    def queue_links(self, n):
        for _ in range(n):
            torch.mm(self.a, self.b, out=self.c)
            self.b, self.c = self.c, self.b

    def queue(self, ms):
        self.queue_links(int(math.ceil(ms / self.ms_per_link)))


_delays = {}


def delay_on(stream):
    if stream.cuda_stream not in _delays:
        _delays[stream.cuda_stream] = Delay(stream)
    return _delays[stream.cuda_stream]


K = 2                                                                         # samples the queued accumulator stands for


def render_call(kernel, n):
    def call(ctx):
        ctx.reset_stats()
        ctx.render(ctx.width, ctx.height, n, seed=SEED, kernel=kernel)
        return ctx.accumulator(), ctx.pixels(), np.uint32([ctx.stats().kernel_launches])
    return call


def reset_then_read(ctx):
    ctx.reset_accumulator()
    return (ctx.accumulator(),)


# case -> (frame, knobs, the call, kernel launches of the render or None); the first device operation of each is of another kind
ORDER_CASES = {
    "megakernel": ((W, H), {}, render_call(P.KERNEL_MEGAKERNEL, 1), 1),                          # a direct launch on the stream
    "persistent_two_streams": ((1024, 512), {"pt_max_paths_mi": 1}, render_call(P.KERNEL_PERSISTENT, 3), 4),   # two batches: the pool streams wait on `begin`
    "wavefront": ((W, H), {}, render_call(P.KERNEL_WAVEFRONT, 2), None),                          # the pool streams wait on `begin`
    "denoise": ((W, H), {}, lambda ctx: ctx.denoise(iterations=2), None),                         # denoise_prepare reads the accumulator
    "accumulator": ((W, H), {}, lambda ctx: (ctx.accumulator(),), None),                          # a drain, then a null-stream copy
    "reset_accumulator": ((W, H), {}, reset_then_read, None),                                     # the queued copy must not land after the memset
}


def queued_data(w, h):
    rng = np.random.default_rng(w * 131 + h)
    a = rng.uniform(0.25, 1.0, (h, w, 4)).astype(np.float32)                  # what a render visibly adds to
    a[..., 3] = np.float32(K)
    return a


def run_ordering_case(scene, stream, name):
    (w, h), knobs, call, launches = ORDER_CASES[name]
    delay = delay_on(stream)
    r, want = on_stream(scene, stream), fresh(scene)
    try:
        zeros, a_host = np.zeros((h, w, 4), np.float32), queued_data(w, h)
        a_dev = torch.from_numpy(a_host).to("cuda:0")
        producer = torch.cuda.current_stream()
        if producer.cuda_stream != stream.cuda_stream:
            stream.wait_stream(producer)                                      # A was made on another stream
        for ctx in (r, want):                                                 # one-time allocations and first launches happen here, not under the delay
            if knobs:
                ctx.set_tuning(**knobs)
            ctx.load_accumulator(zeros, K, w, h)
            call(ctx)
        want.load_accumulator(zeros, K, w, h)
        t0 = time.perf_counter(); call(want); call_ms = 1e3 * (time.perf_counter() - t0)
        r.load_accumulator(zeros, K, w, h)                                    # r's own buffer holds zeros: an early read shows
        ptr, nbytes = r.accumulator_device_ptr()
        assert nbytes == h * w * 16
        view = torch.as_tensor(_DevicePointer(ptr, (h, w, 4)), device="cuda:0")
        target_ms = max(5.0 * call_ms, 20.0)
        assert target_ms <= 250.0, f"{name}: the call alone takes {call_ms:.1f} ms; a delay of five times that is beyond a quarter of a second"
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            start.record(); delay.queue(target_ms); end.record()
            view.copy_(a_dev)
            assert not stream.query(), f"{name}: the delay of {target_ms:.1f} ms was too short: the stream was idle before the call"
            got = call(r)
        want.load_accumulator(a_host, K, w, h)                                # the twin is given the queued data through the host
        ref = call(want)
        end.synchronize()
        delay_ms = start.elapsed_time(end)
        print(f"{name}: delay {delay_ms:.1f} ms on the stream ({delay.ms_per_link:.3f} ms a link), call {call_ms:.2f} ms on the twin")
        same(got, ref, name)
        if name == "reset_accumulator":
            assert not got[0].any()
        elif name == "accumulator":
            same(got, (a_host,), name)
        else:
            assert not np.array_equal(bits(ref[0]), bits(a_host))             # the call did add to, or filter, the queued data
        if launches is not None:
            assert int(ref[2][0]) == launches and int(got[2][0]) == launches
    finally:
        r.close(); want.close()


@pytest.mark.parametrize("lane", range(LANES))
@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_a_call_waits_for_what_was_queued_on_the_callers_stream(world, lanes, name, lane):
    run_ordering_case(world[0], lanes[lane], name)


def run_synchronize(scene, stream):
    delay = delay_on(stream)
    r = on_stream(scene, stream)
    try:
        with torch.cuda.stream(stream):
            delay.queue(20.0)
            assert not stream.query(), "the delay was too short: the stream was idle before synchronize()"
            r.synchronize()
            assert stream.query()
    finally:
        r.close()


def test_synchronize_drains_the_callers_stream(world, side):
    run_synchronize(world[0], side)


# ---- 3. the default stream is refused ---------------------------------------------------------------------------------------------------
# The six cases above were meant to hold on torch's default stream as well, named hipStreamLegacy.  The first run of them on an MI355X
# (ROCm 7.2) passed the megakernel case and ended in a segmentation fault on the host, inside cgpt_render, in the two-stream case of the
# persistent kernel -- the first call that makes a stream wait for an event with hipStreamLegacy in the picture.  So the
# library refuses the default stream under each of its names, and these tests pin the refusals: it never runs unordered in silence.
def default_stream():
    S0 = torch.cuda.current_stream()
    assert S0.cuda_stream == 0 and S0 == torch.cuda.default_stream()         # torch's default stream is the null handle here
    return S0


def test_the_default_stream_is_refused_and_the_stream_that_was_set_stays(world, side):
    s, _ = world
    r, want = on_stream(s, side), fresh(s)
    L = N.lib()
    try:
        ref = frames(want, sizes=SIZE, configs=KERNELS[:2])
        for handle in (default_stream(), default_stream().cuda_stream, 0, np.int64(0)):
            with pytest.raises(ValueError, match="use a non-default stream"):
                r.set_stream(handle)
        for handle, name in ((N.HIP_STREAM_LEGACY, "hipStreamLegacy"), (N.HIP_STREAM_PER_THREAD, "hipStreamPerThread")):
            with pytest.raises(P.DeviceError, match=f"{name} names a default stream; use a non-default stream") as e:
                r.set_stream(handle)
            assert e.value.code == N.CGPT_ERR_UNSUPPORTED
            assert L.cgpt_set_stream(r._ctx, C.c_void_p(handle)) == N.CGPT_ERR_UNSUPPORTED
        with pytest.raises((TypeError, ValueError)):
            r.set_stream("stream")
        delay = delay_on(side)                                                # still on S: synchronize() drains what is queued there
        with torch.cuda.stream(side):
            delay.queue(20.0)
            assert not side.query(), "the delay was too short: the stream was idle before synchronize()"
            r.synchronize()
            assert side.query()
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:2]), ref)
        r.set_stream(None)                                                    # the ABI's null handle: the own stream
        assert L.cgpt_set_stream(r._ctx, None) == N.CGPT_OK
        with torch.cuda.stream(side):
            delay.queue(20.0)
            r.synchronize()                                                   # no longer S's business
            assert not side.query(), "the delay was too short to show that synchronize() left the stream alone"
        side.synchronize()
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:2]), ref)
    finally:
        r.close(); want.close()


def test_set_stream_takes_a_handle_or_a_stream_object(world, side):
    s, _ = world
    r, want = fresh(s), fresh(s)
    try:
        ref = frames(want, sizes=SIZE, configs=KERNELS[:2])
        for stream in (side, side.cuda_stream, None, torch.cuda.Stream(), None):
            r.set_stream(stream)
            assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:2]), ref)
    finally:
        r.close(); want.close()


# ---- 4. switching, sharing and refusing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", THREE_KERNELS)
def test_switching_streams_in_the_middle_of_an_accumulation(world, side, kernel):
    s, _ = world
    r, want = fresh(s), fresh(s)
    try:
        want.render(W, H, 5, seed=SEED, kernel=kernel)
        r.render(W, H, 2, seed=SEED, kernel=kernel)
        r.set_stream(side)
        r.render(W, H, 1, seed=SEED, kernel=kernel)                           # first_sample = 2
        r.set_stream(None)
        r.render(W, H, 2, seed=SEED, kernel=kernel)                           # first_sample = 3
        same((r.accumulator(), r.pixels()), (want.accumulator(), want.pixels()), "2 + 1 + 2 samples")
        assert r.num_accumulated == 5 and r.stats().num_accumulated == 5
    finally:
        r.close(); want.close()


def interleaved(world, streams):
    """two contexts on `streams`, their calls interleaved -- renders by every kernel with a pose batch between them -- each against a twin"""
    s, binds = world
    rs, wants = [on_stream(s, st) for st in streams], [fresh(s), fresh(s)]
    try:
        cases = [BATCH.install(ctx, binds) for ctx in rs + wants][0]
        poses = (entries_of(cases), entries_of(eased(cases, 0.5)))            # each context its own pose
        got, ref = [[], []], [[], []]
        for step, kernel in enumerate(THREE_KERNELS + (P.KERNEL_AUTO,)):
            for k in (0, 1):
                if step == 1:
                    rs[k].pose_objects(poses[k])
                rs[k].reset_accumulator()
                rs[k].render(W, H, 2 + k, seed=SEED + k, kernel=kernel)
            for k in (1, 0):
                got[k].append((rs[k].accumulator(), rs[k].pixels()))
        for k in (0, 1):
            for step, kernel in enumerate(THREE_KERNELS + (P.KERNEL_AUTO,)):
                if step == 1:
                    wants[k].pose_objects(poses[k])
                wants[k].reset_accumulator()
                wants[k].render(W, H, 2 + k, seed=SEED + k, kernel=kernel)
                ref[k].append((wants[k].accumulator(), wants[k].pixels()))
        for k in (0, 1):
            for step in range(4):
                same(got[k][step], ref[k][step], (k, step))
            assert not np.array_equal(bits(ref[k][0][0]), bits(ref[k][1][0]))  # the batch moved something
            for obj in MESHES:
                assert np.array_equal(rs[k].export_bvh(obj), wants[k].export_bvh(obj))
    finally:
        for ctx in rs + wants:
            ctx.close()


def test_two_contexts_on_one_callers_stream(world, side):
    interleaved(world, (side, side))


def test_two_contexts_on_two_callers_streams(world, side):
    other = torch.cuda.Stream()
    assert other.cuda_stream not in (0, side.cuda_stream)
    interleaved(world, (side, other))


def test_a_group_owns_its_streams(world, side):
    s, _ = world
    g, one = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY), fresh(s)
    try:
        for stream in (side, None):
            with pytest.raises(P.DeviceError, match="owns its streams") as e:
                g.set_stream(stream)
            assert e.value.code == N.CGPT_ERR_UNSUPPORTED
        cfg = [(P.KERNEL_WAVEFRONT, None), (P.KERNEL_PERSISTENT, None)]
        assert_same_frames(frames(g, sizes=SIZE, configs=cfg), frames(one, sizes=SIZE, configs=cfg))
        L = N.lib()
        assert L.cgpt_set_stream(None, None) == N.CGPT_ERR_INVALID
    finally:
        g.close(); one.close()


def test_closing_leaves_the_stream_the_callers(world, side):
    s, _ = world
    r = on_stream(s, side)
    r.render(W, H, 2, seed=SEED)
    r.close()
    with torch.cuda.stream(side):
        x = torch.arange(1024, device="cuda:0", dtype=torch.float32) * 2
    side.synchronize()
    assert side.query() and float(x.sum().item()) == 1023 * 1024


# ---- 5. device pointers ---------------------------------------------------------------------------------------------------------------
def device_views(ctx, rows, width):
    ptr, nbytes = ctx.accumulator_device_ptr()
    assert nbytes == rows * width * 16
    acc = torch.as_tensor(_DevicePointer(ptr, (rows, width, 4)), device="cuda:0")
    pptr, pbytes = ctx.pixels_device_ptr()
    assert pbytes == rows * width * 4 and pptr != ptr
    px = torch.as_tensor(_DevicePointer(pptr, (rows, width), "<u4"), device="cuda:0")
    assert acc.data_ptr() == ptr and px.data_ptr() == pptr
    return acc.cpu().numpy(), px.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("where", ["own", "side"])
def test_device_pointers_show_the_accumulator_and_the_pixels(world, side, where):
    s, _ = world
    r = P.Renderer(0)
    try:
        if where == "side":
            r.set_stream(side)
        for call in (r.accumulator_device_ptr, r.pixels_device_ptr):
            with pytest.raises(P.DeviceError, match="nothing rendered yet") as e:
                call()
            assert e.value.code == N.CGPT_ERR_INVALID
        r.upload(s)
        for call in (r.accumulator_device_ptr, r.pixels_device_ptr):
            with pytest.raises(P.DeviceError, match="nothing rendered yet"):
                call()
        seen = []
        for st in (P.Settings(), P.Settings(debug_render_mode=P.DEBUG_BVH_DEPTH)):
            r.reset_accumulator()
            r.render(W, H, 2, seed=SEED, settings=st)
            acc, px = device_views(r, H, W)
            same((acc, px), (r.accumulator(), r.pixels()), ("views", st.debug_render_mode))
            seen.append(px)
        assert seen[0].any() and not np.array_equal(seen[0], seen[1])         # the debug view wrote pixels of its own
        r.render(W, H, 2, seed=SEED, rows=(5, 30))                            # a band: rows * W
        same(device_views(r, 25, W), (r.accumulator(), r.pixels()), "a band")
    finally:
        r.close()


def test_device_pointers_of_a_group_show_the_gathered_frame(world):
    s, _ = world
    g, one = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY), fresh(s)
    try:
        for st in (P.Settings(), P.Settings(debug_render_mode=P.DEBUG_BVH_DEPTH)):
            for ctx in (g, one):
                ctx.reset_accumulator()
                ctx.render(W, H, 2, seed=SEED, settings=st)
            views = device_views(g, H, W)
            same(views, (g.accumulator(), g.pixels()), ("the group's own read-back", st.debug_render_mode))
            same(views, (one.accumulator(), one.pixels()), ("a single context", st.debug_render_mode))
    finally:
        g.close(); one.close()
