"""Reloading a network slot of a live context (nerf_networks.cpp upload_network): every stream of the slot is replaced, a stream the new
network cannot have (the two f16 streams when a weight exceeds the f16 range) is released and its arithmetic refused on the host, and
loading the first network again brings back its bits.  Shapes: forward_batch on 256 points (one tile of the widest kernel, two of the
f32 kernel), renders of a 16 x 8 window with 32 + 32 samples."""
import os

import numpy as np
import pytest

from fold_utils import write_random_net

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16", "bf16x3", "f16x2")
CROP = (24, 28, 16, 8)


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """(random network, the same with viewdirs_kernel[10][3] = 1e5: beyond the f16 range, and only the colours depend on it)"""
    a = write_random_net(tmp_path_factory.mktemp("reload") / "a", 4711)
    b = write_random_net(tmp_path_factory.mktemp("reload") / "b", 4711)
    p = os.path.join(b, "viewdirs_kernel.bin")
    w = np.fromfile(p, "<f4"); w[10 * 128 + 3] = 1e5; w.tofile(p)
    return a, b


def _load(native, r, d):
    r.coarse, r.fine = native.load_network_from_dir(r, 0, d), native.load_network_from_dir(r, 1, d)


def _forward(r, pts, dirs, dtypes):
    out = {}
    for dt in dtypes:
        out[dt] = r.fine.forward_batch(pts, dirs, dtype=dt)
        again = r.coarse.forward_batch(pts, dirs, dtype=dt)                        # both slots hold the same weights
        assert np.array_equal(out[dt][0], again[0]) and np.array_equal(out[dt][1], again[1]), dt
        assert np.isfinite(out[dt][1]).all(), dt
    return out


def _same(x, y):
    return all(np.array_equal(x[dt][k], y[dt][k]) for dt in y for k in (0, 1))


def _certified_equals_plain(native, r, cam):
    plain = native.render_image(r.coarse, r.fine, cam, 32, seed=1, crop=CROP)
    cert, st = native.render_image(r.coarse, r.fine, cam, 32, seed=1, crop=CROP, certify_zero=True, return_stats=True)
    assert np.isfinite(plain).all() and np.array_equal(cert, plain)
    return st


def test_reload_replaces_every_stream_and_refuses_what_the_new_network_lacks(native, samples, nets):
    a, b = nets
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1.5, 1.5, size=(3, 256)).astype(np.float32)
    v = rng.normal(size=(256, 3)); dirs = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    cam = native.camera_from_samples(samples, 64, 64, 32)
    with native.Renderer(0) as fresh:                                              # a context that only ever saw the variant
        _load(native, fresh, b)
        want_b = _forward(fresh, pts, dirs, DTYPES[:3])
    with native.Renderer(0) as r:
        _load(native, r, a)
        first = _forward(r, pts, dirs, DTYPES)
        assert not np.array_equal(first["f32"][0], want_b["f32"][0])                 # the 1e5 weight shows in the colours
        _certified_equals_plain(native, r, cam)

        _load(native, r, b)                                                        # into the same slots
        with pytest.raises(native.NerfError) as e:
            r.fine.forward_batch(pts, dirs, dtype="f16x2")
        assert e.value.code == -6 and e.value.msg == "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range"
        with pytest.raises(native.NerfError) as e:
            native.render_image(r.coarse, r.fine, cam, 32, seed=1, crop=CROP, dtype="f16x2")
        assert e.value.code == -6 and "NERF_MLP_F16X2 is unavailable" in e.value.msg
        assert _same(_forward(r, pts, dirs, DTYPES[:3]), want_b)
        st = _certified_equals_plain(native, r, cam)
        assert st.certify_margin[0] >= 1.0 and st.certify_margin[1] >= 3.0          # the bf16 pre-filter's floors: the f16 twin is gone with its stream

        with pytest.raises(native.NerfError):                                      # a load refused on the host touches nothing
            native.load_network_from_dir(r, 1, os.path.join(a, "missing"))
        assert _same(_forward(r, pts, dirs, DTYPES[:3]), want_b)

        _load(native, r, a)
        assert _same(_forward(r, pts, dirs, DTYPES), first)
        _certified_equals_plain(native, r, cam)
