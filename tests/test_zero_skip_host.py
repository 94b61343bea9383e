"""Host side of zero-step skipping (no GPU): the loaders allow the f32 kernels to skip k-steps whose ReLU inputs are all zero only for a
network whose folded image -- weight stream and small block -- is finite throughout, because fma(a, 0, c) = c needs a finite a
(host_util.cpp zero_skip_safe, asked through nerf_debug_zero_skip_network_dir)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import write_random_net


def _eligible(native, d):
    e = C.c_int(-1)
    assert native.load_library().nerf_debug_zero_skip_network_dir(str(d).encode(), C.byref(e)) == 0
    return e.value


def test_real_and_random_networks_are_eligible(native, tmp_path):
    assert _eligible(native, os.path.join(SCENE, "coarse")) == 1 and _eligible(native, os.path.join(SCENE, "fine")) == 1
    assert _eligible(native, write_random_net(tmp_path / "net", 3)) == 1


# one non-finite value anywhere the f32 kernels read: a trunk weight, a bias, a head weight, and the two layers that reach the stream
# only through the fold (W' = W_b . W_v)
@pytest.mark.parametrize("tensor", ("dense0_kernel", "dense3_kernel", "dense5_bias", "alpha_kernel", "alpha_bias", "rgb_kernel",
                                    "bottleneck_kernel", "bottleneck_bias", "viewdirs_kernel", "viewdirs_bias"))
@pytest.mark.parametrize("value", (np.inf, -np.inf, np.nan))
def test_one_nonfinite_value_switches_the_skip_off(native, tmp_path, tensor, value):
    d = write_random_net(tmp_path / "net", 5)
    path = os.path.join(d, tensor + ".bin")
    a = np.fromfile(path, dtype="<f4")
    a[a.size // 3] = value
    a.tofile(path)
    assert _eligible(native, d) == 0


def test_missing_arguments_are_refused(native, tmp_path):
    L = native.load_library()
    e = C.c_int(-1)
    assert L.nerf_debug_zero_skip_network_dir(None, C.byref(e)) != 0
    assert L.nerf_debug_zero_skip_network_dir(str(tmp_path / "absent").encode(), C.byref(e)) != 0
    assert L.nerf_debug_zero_skip_network_dir(os.path.join(SCENE, "fine").encode(), None) != 0
