"""CPU sanitizer run of the host-only half of the C ABI (`make -C nerf-rs_amd/csrc host-asan`: nerf_host_api.cpp + host_util.cpp under
AddressSanitizer + UBSan, plain clang++, no HIP).  Everything in the product that parses bytes from disk lives there: shapes.txt /
<name>.bin loader (reference src/lib.rs:34-74, 108-174), the packed-blob reader, the hand-written camera JSON reader
(src/lib.rs:614-645), the PPM writer and quantisers (src/lib.rs:567-592), the operand splitters.  Each case must come back with a
status code; a sanitizer report (heap overflow, UB, leak) aborts the driver with a non-zero exit and fails the test.
GPU ASan is not available on this pool, and none of this code touches the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE

CSRC = os.path.join(ROOT, "nerf-rs_amd", "csrc")
DRIVER = os.path.join(CSRC, "build", "host_asan_driver")


@pytest.fixture(scope="module")
def asan():
    subprocess.check_call(["make", "-s", "-C", CSRC, "host-asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=87", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(*args):
        p = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, f"{args}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
        last = p.stdout.strip().splitlines()[-1]
        rc = int(last.split("rc=")[1].split()[0])
        return rc, last.split("msg=", 1)[1], p.stdout
    return run


def test_valid_inputs_under_sanitizers(asan, tmp_path):
    for net in ("coarse", "fine"):
        assert asan("check_dir", os.path.join(SCENE, net))[0] == 0
        rc, _, out = asan("debug_pack", os.path.join(SCENE, net))
        assert rc == 0 and "packed 593920 + 3136 floats" in out
        rc, _, out = asan("streams_dir", os.path.join(SCENE, net))
        assert rc == 0 and "stream 0: 598016 elements, available 1" in out and "stream 1: 598016 elements, available 1" in out
        assert "stream 2: 1781760 elements, available 1" in out and "stream 3: 1187840 elements, available 1" in out
        blob = tmp_path / f"{net}.nrf"
        assert asan("pack_dir", os.path.join(SCENE, net), blob)[0] == 0
        assert asan("check_blob", blob)[0] == 0
    rc, _, out = asan("camera_json", os.path.join(SCENE, "tf_reference_samples.json"), 800, 800)
    assert rc == 0 and "camera 800 800" in out and "near 2 far 6" in out
    rc, _, out = asan("quantize")
    assert rc == 0 and out.splitlines()[0].startswith("0 0 128 255 255 0 255 0 0 255 64 191 | 0 0 128 255 255 255 0 255")
    assert asan("split")[0] == 0
    assert asan("save_ppm", tmp_path / "a.ppm", 7, 5)[0] == 0 and (tmp_path / "a.ppm").stat().st_size == 11 + 105
    assert asan("save_ppm", tmp_path / "b.ppm", 0, 5)[0] == -1
    assert asan("save_ppm", tmp_path / "b.ppm", -3, -5)[0] == -1
    assert asan("save_ppm", tmp_path / "no" / "dir" / "b.ppm", 2, 2)[0] == -2


def test_stage_layout_under_sanitizers(asan):
    """stage_layout.h, the bump allocator of every staging layout and pass workspace: parts absent and present, a zero-length part, a
    guarded part, the alignment of every offset, the total, and sizes beyond size_t refused instead of wrapped (the driver's checks: rc
    names the first that failed)."""
    rc, msg, out = asan("stage_layout")
    assert rc == 0 and "stage_layout total 1792 parts 5" in out, (rc, msg, out)


def test_malformed_weight_directories(asan, tmp_path):
    src = os.path.join(SCENE, "coarse")
    good_shapes = open(os.path.join(src, "shapes.txt")).read()
    d = tmp_path / "net"

    def fresh():
        if d.exists():
            shutil.rmtree(d)
        shutil.copytree(src, d)

    assert asan("check_dir", tmp_path / "nope")[0] == -2
    # shapes.txt variants: truncated mid-line, empty, garbage, absurd / negative / non-numeric dimensions, a very long line
    variants = {
        "truncated": good_shapes[:len(good_shapes) // 2 - 3],
        "empty": "",
        "blank lines": "\n\n \n" + good_shapes,
        "huge dims": good_shapes.replace("dense0_kernel 63 256", "dense0_kernel 99999999999999 99999999999999"),
        "overflowing dim": good_shapes.replace("dense0_kernel 63 256", "dense0_kernel 99999999999999999999999999 256"),
        "negative dim": good_shapes.replace("dense1_bias 256", "dense1_bias -256"),
        "non-numeric": good_shapes.replace("dense1_bias 256", "dense1_bias 25x6"),
        "three dims": good_shapes.replace("dense0_kernel 63 256", "dense0_kernel 63 256 1"),
        "no dims": good_shapes.replace("dense0_kernel 63 256", "dense0_kernel"),
        "swapped dims": good_shapes.replace("dense0_kernel 63 256", "dense0_kernel 256 63"),
        "zero dims": good_shapes.replace("alpha_bias 1", "alpha_bias 0"),
        "long line": "x" * 70000 + " 4\n" + good_shapes,
        "path escape": "../coarse/dense0_kernel 63 256\n" + good_shapes,
        "binary": bytes(range(256)).decode("latin-1") * 40,
    }
    for name, text in variants.items():
        fresh()
        (d / "shapes.txt").write_bytes(text.encode("latin-1"))
        rc, msg, _ = asan("check_dir", d)
        assert rc in (0, -2, -3, -4, -7), (name, rc, msg)
        if name in ("huge dims", "overflowing dim", "negative dim", "non-numeric", "three dims", "no dims", "swapped dims", "zero dims", "empty", "truncated"):
            assert rc != 0, (name, msg)
        assert asan("pack_dir", d, tmp_path / "x.nrf")[0] == rc
        assert asan("streams_dir", d)[0] == rc
    # tensor files: truncated, empty, oversized by a few bytes, oversized by a lot, not a multiple of four
    for name, data in {"half": None, "empty": b"", "plus3": b"\1\2\3", "odd": b"\0" * 5}.items():
        fresh()
        p = d / "dense4_kernel.bin"
        raw = p.read_bytes()
        p.write_bytes(raw[:len(raw) // 2] if data is None else (raw + data if name != "empty" else b""))
        rc, msg, _ = asan("check_dir", d)
        assert (rc == 0) == (name == "plus3"), (name, rc, msg)  # chunks_exact(4) ignores a ragged tail of < 4 bytes (src/lib.rs:38-41)
        assert rc in (0, -4), (name, rc, msg)
    fresh()
    with open(d / "rgb_bias.bin", "ab") as f:
        f.write(b"\0" * (1 << 20))
    assert asan("check_dir", d)[0] == -4


def test_streams_of_a_network_beyond_the_f16_range(asan, tmp_path):
    """build_streams with a weight of 1e5 and a NaN weight: the two f16 streams are unavailable (no elements), the two bf16 streams are built."""
    for value in (1e5, np.nan):
        d = tmp_path / f"net_{value}"
        shutil.copytree(os.path.join(SCENE, "coarse"), d)
        w = np.fromfile(d / "dense5_kernel.bin", "<f4"); w[12345] = value; w.tofile(d / "dense5_kernel.bin")
        rc, _, out = asan("streams_dir", d)
        assert rc == 0 and "stream 0: 598016 elements, available 1" in out and "stream 2: 1781760 elements, available 1" in out, out
        assert "stream 1: 0 elements, available 0" in out and "stream 3: 0 elements, available 0" in out, out


def test_malformed_blobs(asan, tmp_path):
    blob = tmp_path / "c.nrf"
    assert asan("pack_dir", os.path.join(SCENE, "coarse"), blob)[0] == 0
    raw = blob.read_bytes()
    bad = tmp_path / "bad.nrf"
    for cut in (0, 1, 7, 8, 12, 15, 16, 17, 1000, len(raw) // 2, len(raw) - 4, len(raw) - 1):
        bad.write_bytes(raw[:cut])
        assert asan("check_blob", bad)[0] == -4, cut
    for name, data in {"trailing byte": raw + b"\0", "trailing MB": raw + b"\1" * (1 << 20), "magic": b"NRFMI356" + raw[8:],
                       "version": raw[:8] + np.uint32(2).tobytes() + raw[12:], "count small": raw[:12] + np.uint32(16).tobytes() + raw[16:],
                       "count huge": raw[:12] + np.uint32(0xffffffff).tobytes() + raw[16:]}.items():
        bad.write_bytes(data)
        assert asan("check_blob", bad)[0] == -4, name
    assert asan("check_blob", tmp_path / "missing.nrf")[0] == -2
    assert asan("check_blob", tmp_path)[0] in (-2, -4)  # a directory


def test_malformed_camera_json(asan, tmp_path):
    good = open(os.path.join(SCENE, "tf_reference_samples.json")).read().rstrip()
    p = tmp_path / "cam.json"
    n_ok = 0
    for cut in list(range(0, len(good), 997)) + [len(good) - 2, len(good) - 1]:
        p.write_text(good[:cut])
        rc, msg, _ = asan("camera_json", p, 64, 64)
        assert rc in (0, -7), (cut, rc, msg)
        n_ok += rc == 0
    assert n_ok == 0  # every proper prefix is refused
    cases = {
        "deep arrays": "{\"near\": " + "[" * 100000 + "1" + "]" * 100000 + "}",
        "deep objects": "{\"a\": " + "{\"a\": " * 5000 + "1" + "}" * 5000 + "}",
        "huge numbers": good.replace("2.0", "1e999999", 1),
        "many numbers": "{\"near\": 2, \"far\": 6, \"hwf\": [" + ", ".join(["1.5"] * 200000) + "], \"camera_origin\": [0,0,0], \"camera_forward\": [0,0,-1], \"camera_up\": [0,1,0]}",
        "short hwf": "{\"near\": 2, \"far\": 6, \"hwf\": [400, 400], \"camera_origin\": [0,0,0], \"camera_forward\": [0,0,-1], \"camera_up\": [0,1,0]}",
        "strings for numbers": "{\"near\": \"2\", \"far\": 6, \"hwf\": [400, 400, 555], \"camera_origin\": [0,0,0], \"camera_forward\": [0,0,-1], \"camera_up\": [0,1,0]}",
        "unterminated string": "{\"near",
        "escape at end": "{\"near\\",
        "nul bytes": "{\"near\": 2\0, \"far\": 6}",
        "not an object": "[1, 2, 3]",
        "empty": "",
        "whitespace": " \n\t ",
        "zero focal": "{\"near\": 2, \"far\": 6, \"hwf\": [400, 400, 0], \"camera_origin\": [0,0,0], \"camera_forward\": [0,0,0], \"camera_up\": [0,0,0]}",
        "nan tokens": "{\"near\": nan, \"far\": inf, \"hwf\": [400, 400, 555], \"camera_origin\": [0,0,0], \"camera_forward\": [0,0,-1], \"camera_up\": [0,1,0]}",
    }
    for name, text in cases.items():
        p.write_bytes(text.encode())
        rc, msg, _ = asan("camera_json", p, 64, 64)
        assert rc in (0, -7), (name, rc, msg)
        if name not in ("many numbers", "zero focal", "nan tokens", "huge numbers"):
            assert rc == -7, (name, msg)
    assert asan("camera_json", tmp_path / "missing.json", 8, 8)[0] == -2
    assert asan("camera_json", os.path.join(SCENE, "tf_reference_samples.json"), 0, -5)[0] == 0  # sizes are checked at render time (src/lib.rs:705-709)
