"""Host side of the RGBA8 output: nerf_save_pam (P7, TUPLTYPE RGB_ALPHA -- the Netpbm format that holds an alpha channel), through the
library and, under AddressSanitizer + UBSan, through the stand-alone host driver (`make host-asan`).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _header(w, h):
    return f"P7\nWIDTH {w}\nHEIGHT {h}\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n".encode()


def _read_pam(path):
    raw = open(path, "rb").read()
    head, data = raw.split(b"ENDHDR\n", 1)
    fields = dict(l.split(b" ", 1) for l in head.split(b"\n")[1:] if l)
    w, h = int(fields[b"WIDTH"]), int(fields[b"HEIGHT"])
    assert head.startswith(b"P7\n") and fields[b"DEPTH"] == b"4" and fields[b"MAXVAL"] == b"255" and fields[b"TUPLTYPE"] == b"RGB_ALPHA"
    return np.frombuffer(data, np.uint8).reshape(h, w, 4)


def test_save_pam_writes_the_exact_header_and_bytes(native, tmp_path):
    img = (np.arange(3 * 2 * 4, dtype=np.uint32) * 37 + 11).astype(np.uint8).reshape(2, 3, 4)   # 3 wide, 2 high
    path = tmp_path / "a.pam"
    native.save_pam(path, 3, 2, img)
    assert path.read_bytes() == _header(3, 2) + img.tobytes()
    assert np.array_equal(_read_pam(path), img)
    one = np.array([[[1, 2, 3, 4]]], np.uint8)
    native.save_pam(tmp_path / "one.pam", 1, 1, one)
    assert (tmp_path / "one.pam").read_bytes() == _header(1, 1) + bytes([1, 2, 3, 4])


def test_save_pam_errors(native, tmp_path):
    from nerf_rs_amd import _lib
    L = native.load_library()
    img = np.zeros((2, 3, 4), np.uint8)
    p = img.ctypes.data_as(_lib.u8p)
    for w, h in ((0, 2), (3, 0), (-3, 2), (3, -2)):
        assert L.nerf_save_pam(str(tmp_path / "bad.pam").encode(), w, h, p) == -1          # NERF_ERR_INVALID
        assert b"bad size" in L.nerf_last_error(None)
    assert not (tmp_path / "bad.pam").exists()
    assert L.nerf_save_pam(str(tmp_path / "bad.pam").encode(), 3, 2, None) == -1
    assert L.nerf_save_pam(None, 3, 2, p) == -1
    assert L.nerf_save_pam(str(tmp_path / "no" / "such" / "dir" / "a.pam").encode(), 3, 2, p) == -2   # NERF_ERR_IO
    assert b"cannot create" in L.nerf_last_error(None)
    with pytest.raises(native.NerfError):
        native.save_pam(tmp_path / "c.pam", 3, 2, np.zeros((2, 3, 3), np.uint8))          # not width * height * 4 bytes


def test_python_layer_rejects_bad_arguments_without_a_device(native):
    from nerf_rs_amd import api
    assert api._alpha("opaque") == 0 and api._alpha("premultiplied") == 1 and api._alpha("straight") == 2 and api._alpha(2) == 2
    with pytest.raises(native.NerfError):
        api._alpha("additive")
    with pytest.raises(native.NerfError):
        api._background((1.0, 2.0))
    assert api._background(None) == (None, None)
    keep, ptr = api._background((0.25, 0.5, 0.75))
    assert keep.dtype == np.float32 and [ptr[i] for i in range(3)] == [0.25, 0.5, 0.75]
    L = native.load_library()
    assert L.nerf_render_image_rgba8(None, None, None, None, 0, None, None) == -1           # no context: an error code, not a crash
    assert L.nerf_stage_integrate_rgba8(None, 1, 1, 6.0, None, None, None, None, 0, None) == -1


def test_save_pam_under_sanitizers(tmp_path):
    """The stand-alone host driver (AddressSanitizer + UBSan): a 1 x 1 image, a ragged one, bad sizes and an unwritable path.  Its buffer
    holds exactly width x height x 4 bytes, so an over-read of the writer is a sanitizer report."""
    csrc = os.path.join(ROOT, "nerf-rs_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "host-asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=87", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(path, w, h):
        p = subprocess.run([os.path.join(csrc, "build", "host_asan_driver"), "save_pam", str(path), str(w), str(h)],
                           capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
        return int(p.stdout.strip().splitlines()[-1].split("rc=")[1].split()[0])
    assert run(tmp_path / "one.pam", 1, 1) == 0 and (tmp_path / "one.pam").stat().st_size == len(_header(1, 1)) + 4
    assert run(tmp_path / "r.pam", 7, 5) == 0 and (tmp_path / "r.pam").read_bytes().startswith(_header(7, 5))
    assert run(tmp_path / "z.pam", 0, 5) == -1 and run(tmp_path / "z.pam", -3, -5) == -1
    assert run(tmp_path / "no" / "dir" / "b.pam", 2, 2) == -2
