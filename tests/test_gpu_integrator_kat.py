"""The integrators on the device against closed-form answers (integrator_ref.py): every case of tests/test_integrator_reference.py through
P.Renderer with each kernel choice, held to the same acceptance rule (16 quantile bins, 5 sigma of the model's variance plus a 1e-3 floor,
exact zeros bitwise), and the kernels' accumulators compared to the bit.  The scenes with mesh floors or mesh slab faces send the rays
through wf_trace and get_hit's flat normal (SURVEY A-8), the others through the shade kernel's probe."""
import numpy as np
import pytest

import cpugpupathtracing_amd as P
import integrator_ref as R

pytestmark = pytest.mark.gpu

ODD_BATCHES = (61, 37, 13)       # samples per wavefront batch: the first that the case's sample count is no multiple of (a short last batch)
KERNELS = {
    "megakernel": (P.KERNEL_MEGAKERNEL, None),
    "wavefront": (P.KERNEL_WAVEFRONT, None),
    "wavefront_odd_batch": (P.KERNEL_WAVEFRONT, "odd batch"),
    "persistent": (P.KERNEL_PERSISTENT, None),
    "auto": (P.KERNEL_AUTO, None),
}
_rendered = {}


def _accumulator(name, kernel):
    """One render per (case, kernel choice), shared by the tests below and left unchanged."""
    if (name, kernel) not in _rendered:
        c = R.case(name)
        o, s = c.build()
        r = P.Renderer(0)
        try:
            r.upload(s)
            origin = np.broadcast_to(np.asarray(c.camera[0], np.float32), (c.H * c.W, 3))
            t, obj, _, _ = r.intersect_rays(origin, c.rays().reshape(-1, 3).astype(np.float32))
            assert np.all(obj == c.primary_object), "every primary ray must hit the intended surface"
            assert np.allclose(t, c.primary_t.ravel(), rtol=1e-5)
            which, knobs = KERNELS[kernel]
            if knobs:
                batch = next(b for b in ODD_BATCHES if c.spp % b != 0 and c.spp > 2 * b)
                r.set_tuning(batch=batch)
            r.render(c.W, c.H, c.spp, seed=R.SEED, kernel=which, settings=c.settings())
            _rendered[name, kernel] = r.accumulator().copy()
        finally:
            r.close(); o.close(); s.close()
    return _rendered[name, kernel]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_device_matches_the_closed_form(name, kernel):
    R.case(name).check(_accumulator(name, kernel), kernel)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_kernels_agree_to_the_bit(name):
    first = _accumulator(name, "megakernel").view(np.uint32)
    for kernel in KERNELS:
        assert np.array_equal(_accumulator(name, kernel).view(np.uint32), first), (name, kernel)
