"""Random sequences of in-place scene edits on the device against the host model of tests/edit_model.py.

Context A is uploaded once and then given every operation of a seeded sequence, refused calls included.  The yardstick is never a device
edit: after every step A must equal the model's host scene -- the exported trees word for word, the joint matrices of every posed skin
-- and a context B that was created for that step alone, uploaded from the model's scene and given A's top-level switch: one render,
cgpt_intersect_rays and the guides, to the bit.  After the last step the whole contract of tests/test_gpu_rebuild_mesh.py is run between A
and a fresh B.  A step is never retried.  CGPT_EDIT_FUZZ_SEEDS=n adds n seeds to every row of the default set, CGPT_EDIT_FUZZ_STEPS sets
the length of every sequence (default 16); a failing step prints its seed, its index and the operations up to it."""
import os
import time

import numpy as np
import pytest

import cpugpupathtracing_amd as P
import edit_model as E
from test_gpu_rebuild_mesh import KERNELS, MODES, assert_contract
from test_gpu_rebuild_mesh import frames as contract_frames
from test_gpu_refit import assert_same_frames, frames, random_rays
from test_gpu_skinning import bits

pytestmark = pytest.mark.gpu

SETS = E.default_set(int(os.environ.get("CGPT_EDIT_FUZZ_SEEDS", "0")), int(os.environ.get("CGPT_EDIT_FUZZ_STEPS", str(E.STEPS))))
SIZE = ((64, 64),)


def context(kind):
    """context A of a row: default, the slow knobs from the start, or two members on one device"""
    if kind == "group":
        return P.Renderer([0, 0], flags=P.CTX_GATHER_PEER_COPY)
    r = P.Renderer(0)
    if kind == "knobs":
        r.set_tuning(**E.SLOW_KNOBS)
    return r


def yardstick(model):
    """context B: a fresh upload of the model's scene, with the model's top-level switch; none of the sequence's device edits"""
    b = P.Renderer(0)
    b.upload(model.scene, instanced=model.instanced)
    b.set_top_level(model.top_level)
    return b


def assert_trees_and_poses(a, model):
    for obj in model.mesh_objects():
        dev, ref = a.export_bvh(obj), model.scene.bvh_export(obj)[0]
        assert dev.shape == ref.shape, (obj, dev.shape, ref.shape)
        assert np.array_equal(dev, ref), f"object {obj}: {np.count_nonzero(dev != ref)} words of the tree differ from the model's"
    for obj, m in model.posed_skins().items():
        assert np.array_equal(bits(a.joint_matrices(obj, len(m))), bits(m)), f"object {obj}: joint_matrices is not the model's last pose"


def assert_step(a, model, step, rays):
    assert_trees_and_poses(a, model)
    b = yardstick(model)
    try:
        config = [(KERNELS[step % len(KERNELS)], None)]                       # megakernel, wavefront, persistent in turn
        assert_same_frames(frames(a, sizes=SIZE, configs=config), frames(b, sizes=SIZE, configs=config))
        assert np.array_equal(bits(a.guides()), bits(b.guides())), "guides"
        for name, x, y in zip(("t", "obj", "tri", "bvh_depth"), a.intersect_rays(*rays), b.intersect_rays(*rays)):
            assert np.array_equal(bits(x), bits(y)), f"intersect_rays: {np.count_nonzero(bits(x) != bits(y))} values of {name} differ"
    finally:
        b.close()


def assert_final(a, model, is_group, rays):
    b = yardstick(model)
    try:
        if not is_group:
            assert_contract(a, b, model.scene)
            return
        # cgpt_trace_rays serves one-device contexts only: the contract's other parts, from its own pieces
        assert_trees_and_poses(a, model)
        for top in (False, True):
            for ctx in (a, b):
                ctx.set_top_level(top)
            assert_same_frames(contract_frames(a, KERNELS, MODES), contract_frames(b, KERNELS, MODES))
            assert np.array_equal(bits(a.guides()), bits(b.guides())), "guides"
            for x, y in zip(a.intersect_rays(*rays), b.intersect_rays(*rays)):
                assert np.array_equal(bits(x), bits(y))
    finally:
        b.close()


def run_sequence(kind, ctx_kind, ops, label):
    model = E.Model(kind)
    a = context(ctx_kind)
    rays = random_rays(4096, 5)
    done = []
    t0 = time.perf_counter()
    try:
        a.upload(model.scene, instanced=model.instanced)
        for step, op in enumerate(ops):
            status = E.apply_to_model(model, op)
            done.append(f"  {step:2d} {status:8s} {E.describe(op)}")
            try:
                got = E.apply_to_device(a, op, status, model)
                if op[0] == "refit_mesh" and status == "accepted" and model.last_area is not None:
                    assert bits(np.float32(got)) == bits(np.float32(model.last_area)), f"total_area {got} is not the mirror's {model.last_area}"
                assert_step(a, model, step, rays)
            except (AssertionError, P.DeviceError) as e:                     # a read the device refuses (joint_matrices of a skin it holds unposed) is a mismatch too
                raise AssertionError(f"{label}, step {step}:\n" + "\n".join(done) + f"\n{e}") from e
        try:
            assert_final(a, model, ctx_kind == "group", rays)
        except (AssertionError, P.DeviceError) as e:
            raise AssertionError(f"{label}, after the last step:\n" + "\n".join(done) + f"\n{e}") from e
    finally:
        a.close()
        model.close()
    print(f"{label}: {len(ops)} steps in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("kind,ctx_kind,seed,steps", SETS, ids=[f"{k}-{c}-{s}" for k, c, s, _ in SETS])
def test_the_device_equals_a_fresh_upload_of_the_model_after_every_step(kind, ctx_kind, seed, steps):
    ops = E.sequence_of(kind, ctx_kind, seed, steps)
    run_sequence(kind, ctx_kind, ops, f"{kind} scene, {ctx_kind} context, seed {seed}, {steps} steps")
