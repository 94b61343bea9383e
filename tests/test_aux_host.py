"""Depth and opacity maps, host side (no device): nerf_save_pfm round-trips, and the new entry points of nerf_render_image_aux are
declared in every place a caller reads them -- the header, the ctypes table and the Rust `-sys` extern block."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "nerf_mi355x.h")
AUX_FUNCTIONS = ("nerf_render_image_aux", "nerf_render_image_aux_device", "nerf_render_image_multi_aux", "nerf_save_pfm")


def _read_pfm(path):
    raw = open(path, "rb").read()
    head, rest = raw.split(b"\n", 1)
    dims, rest = rest.split(b"\n", 1)
    scale, data = rest.split(b"\n", 1)
    w, h = (int(v) for v in dims.split())
    return head, w, h, float(scale), data


def test_save_pfm_round_trip(native, tmp_path):
    rng = np.random.default_rng(3)
    m = rng.uniform(-2, 7, size=(5, 7)).astype(np.float32)
    m[0, 0], m[4, 6] = 0.0, 1.0000005
    p = tmp_path / "depth.pfm"
    native.save_pfm(p, 7, 5, m)
    head, w, h, scale, data = _read_pfm(p)
    assert (head, w, h, scale) == (b"Pf", 7, 5, -1.0)                       # one channel, negative scale: little-endian
    assert len(data) == 7 * 5 * 4 and p.read_bytes().startswith(b"Pf\n7 5\n-1.0\n")
    back = np.frombuffer(data, "<f4").reshape(5, 7)[::-1]                   # rows stored bottom-up
    assert np.array_equal(back, m)


def test_save_pfm_errors(native, tmp_path):
    L = native.load_library()
    v = np.zeros(4, np.float32)
    ptr = v.ctypes.data_as(native._lib.f32p)
    assert L.nerf_save_pfm(str(tmp_path / "no" / "dir" / "a.pfm").encode(), 2, 2, ptr) == -2   # NERF_ERR_IO
    assert b"cannot create" in L.nerf_last_error(None)
    assert L.nerf_save_pfm(str(tmp_path / "a.pfm").encode(), 0, 2, ptr) == -1                  # NERF_ERR_INVALID
    assert L.nerf_save_pfm(str(tmp_path / "a.pfm").encode(), 2, -1, ptr) == -1
    assert L.nerf_save_pfm(None, 2, 2, ptr) == -1 and L.nerf_save_pfm(str(tmp_path / "a.pfm").encode(), 2, 2, None) == -1
    with pytest.raises(native.NerfError):
        native.save_pfm(tmp_path / "b.pfm", 3, 3, v)                                             # 4 values for 3 x 3


def test_aux_functions_are_declared_everywhere(native):
    from nerf_rs_amd import _lib
    htext = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "nerf-mi355x-sys", "src", "lib.rs")).read()
    block = rs[rs.index('extern "C" {'):]
    L = native.load_library()
    for name in AUX_FUNCTIONS:
        assert re.search(r"\b" + name + r"\s*\(", htext), name
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"pub fn " + name + r"\s*\(", block), name
        assert getattr(L, name) is not None                                  # exported by the library
    assert len(_lib.PROTOTYPES["nerf_render_image_aux"][1]) == len(_lib.PROTOTYPES["nerf_render_image"][1]) + 2
    assert len(_lib.PROTOTYPES["nerf_render_image_multi_aux"][1]) == len(_lib.PROTOTYPES["nerf_render_image_multi"][1]) + 2
    assert "render_image_aux" in open(os.path.join(ROOT, "bindings", "rust", "nerf-mi355x", "src", "lib.rs")).read()
    assert "save_pfm" in native.__dict__


def test_host_asan_save_pfm(tmp_path):
    """The PFM writer lives in the HIP-free host half: it runs under ASan + UBSan like the PPM writer."""
    import subprocess
    csrc = os.path.join(ROOT, "nerf-rs_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "host-asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=87", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(*args):
        p = subprocess.run([os.path.join(csrc, "build", "host_asan_driver"), "save_pfm"] + [str(a) for a in args],
                           capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0 and "runtime error" not in p.stderr, p.stderr[-4000:]
        return int(p.stdout.strip().splitlines()[-1].split("rc=")[1].split()[0])
    assert run(tmp_path / "a.pfm", 9, 4) == 0
    head, w, h, scale, data = _read_pfm(tmp_path / "a.pfm")
    assert (head, w, h, scale, len(data)) == (b"Pf", 9, 4, -1.0, 9 * 4 * 4)
    first_row = np.frombuffer(data, "<f4").reshape(4, 9)[-1]
    assert np.array_equal(first_row, np.arange(9, dtype=np.float32) * 0.0625 - 1.5)
    assert run(tmp_path / "b.pfm", 0, 4) == -1
    assert run(tmp_path / "no" / "dir" / "b.pfm", 2, 2) == -2
