"""The per-workgroup clock diagnostic (NERF_DEBUG_CLOCK, nerf_debug_workgroup_clocks, nerf_debug_shader_clock_mhz): every persistent workgroup
of the fine (1) or the sampling (2) f32 launch stamps its tile loop; tools/workgroup_spread.py reads a launch's load balance from it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_zero_skip import _env  # noqa: E402  (its helper, not its tests)

pytestmark = pytest.mark.gpu

CROP = (272, 300, 256, 16)     # 4 096 rays: 2 048 coarse and 6 144 fine tiles, several rounds for each of the 256 workgroups


def _renderer(native, value):
    with _env(value, "NERF_DEBUG_CLOCK"):
        r = native.Renderer(0)
    r.load_scene(SCENE)
    return r


@pytest.mark.parametrize("mode", ("1", "2"))
def test_clocks_of_the_fine_and_of_the_sampling_launch(native, samples, mode):
    cam = native.camera_from_samples(samples, 800, 800, 64)
    with _renderer(native, mode) as r:
        n_cus = r.device_info()["n_cus"]
        buf = np.zeros(2 * (n_cus + 1), np.uint64)
        p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
        assert r._L.nerf_debug_workgroup_clocks(r.handle, p, n_cus) != 0        # no frame rendered yet
        native.render_image(r.coarse, r.fine, cam, 128, seed=0, crop=CROP)
        clocks = r.workgroup_clocks()
        assert clocks.shape == (n_cus, 2) and (clocks > 0).all()
        mhz = C.c_double()
        assert r._L.nerf_debug_shader_clock_mhz(r.handle, C.byref(mhz)) == 0 and 500.0 < mhz.value < 3000.0
        ms = clocks[:, 1].astype(np.float64) / 1e5                               # 100 MHz ticks
        assert ms.max() < 1000.0 and ms.max() / ms.mean() < 2.0
        assert r._L.nerf_debug_workgroup_clocks(r.handle, p, n_cus + 1) != 0    # more workgroups than the context launches
        assert r._L.nerf_debug_workgroup_clocks(r.handle, None, n_cus) != 0
        assert not buf.any()


def test_the_sampling_launch_is_the_shorter_one(native, samples):
    """Mode 2 really is the other launch: 64 sigma-only samples per ray against 192 full ones."""
    cam = native.camera_from_samples(samples, 800, 800, 64)
    mean = {}
    for mode in ("1", "2"):
        with _renderer(native, mode) as r:
            for _ in range(2):
                native.render_image(r.coarse, r.fine, cam, 128, seed=0, crop=CROP)
            mean[mode] = r.workgroup_clocks()[:, 1].astype(np.float64).mean()
    assert mean["2"] < 0.6 * mean["1"], mean


def test_without_the_variable_there_are_no_clocks(native, samples):
    cam = native.camera_from_samples(samples, 800, 800, 64)
    with _renderer(native, None) as r:
        native.render_image(r.coarse, r.fine, cam, 128, seed=0, crop=(300, 310, 8, 4))
        with pytest.raises(native.NerfError):
            r.workgroup_clocks()
