"""Density queries on the GPU: nerf_density_batch (sigma alone at caller points) and nerf_density_grid (sigma and / or packed occupancy
on a lattice whose points the kernel generates itself), against nerf_forward_batch, the live CPU oracle and NumPy restatements.

Stated tolerances: none between the library's own entry points -- density_batch, the lattice grid and forward_batch's sigma run the same
trunk instruction sequence and the same alpha head on the same f32 point bits, so they must agree BIT FOR BIT; against the oracle the
project's forward_batch gate, |dsigma| <= 1e-4 (1 + |sigma|).  The occupancy words, their count and their bounds are exact integer
functions of the GPU's own sigma grid.

The lattices: single cell; less than one 32-point wave tile (one partial word); exactly one 128-point workgroup tile; nx not a multiple
of 32 with a ragged last tile and word; another ragged last tile; and 272 tiles -- more than one persistent grid of 256 workgroups, so the
tile loop runs twice in some of them."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE, golden

pytestmark = pytest.mark.gpu

SIGMA_TOL = 1e-4
LATTICES = [
    ((0.0, 0.0, 0.2), (0.1, 0.1, 0.1), (1, 1, 1)),
    ((-0.5, -0.9, 0.0), (0.25, 0.9, 0.5), (5, 3, 2)),
    ((-0.62, -1.1, -0.1), (0.04, 0.7, 0.5), (32, 4, 1)),
    ((-0.7, -1.2, -0.6), (0.045, 0.35, 0.6), (33, 7, 3)),
    ((-0.6, -1.0, -0.2), (0.07, 0.25, 0.3), (17, 9, 5)),
    ((-1.3, -1.3, -0.8), (0.0667, 0.0897, 0.0679), (40, 30, 29)),
]
LATTICE_IDS = ["x".join(str(d) for d in lat[2]) for lat in LATTICES]
NETS = ["coarse", "fine"]
THRESHOLDS = [0.0, 10.0, 1e9]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def lattice_points(lo, step, dims):
    """(3, N) float32, x fastest: per coordinate the f32 product step * (float)index, then the f32 sum with lo, each rounded once."""
    nx, ny, nz = dims
    axes = [np.float32(lo[k]) + np.float32(step[k]) * np.arange(dims[k], dtype=np.float32) for k in range(3)]
    assert all(a.dtype == np.float32 for a in axes)
    return np.stack([np.tile(axes[0], ny * nz), np.tile(np.repeat(axes[1], nx), nz), np.repeat(axes[2], nx * ny)]).astype(np.float32)


class DeviceBuffers:
    """Device memory for the *_device entry points, through the HIP runtime the library itself is linked against (looked up through the
    library's handle), so that the tests need no second GPU stack in the process."""

    def __init__(self, native):
        import ctypes as C
        L = native.load_library()
        self._C = C
        self._malloc, self._free, self._memcpy, self._sync = L.hipMalloc, L.hipFree, L.hipMemcpy, L.hipDeviceSynchronize
        self._malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self._free.argtypes = [C.c_void_p]
        self._memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for f in (self._malloc, self._free, self._memcpy, self._sync):
            f.restype = C.c_int
        self._live = []

    def upload(self, array):
        a = np.ascontiguousarray(array)
        p = self._C.c_void_p()
        assert self._malloc(self._C.byref(p), max(a.nbytes, 4)) == 0
        self._live.append(p.value)
        assert self._memcpy(p.value, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice
        return p.value

    def download(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        assert self._sync() == 0
        assert self._memcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0            # hipMemcpyDeviceToHost
        return out

    def close(self):
        for p in self._live:
            self._free(p)
        self._live = []


@pytest.fixture
def device(native, renderer):
    d = DeviceBuffers(native)
    yield d
    d.close()


def _net(renderer, name):
    return renderer.coarse if name == "coarse" else renderer.fine


def _oracle_sigma(oracle_nets, name, pts):
    dirs = np.tile(np.float32([0.0, 0.0, 1.0]), (pts.shape[1], 1))          # density does not depend on the direction
    return (oracle_nets[0] if name == "coarse" else oracle_nets[1]).forward_batch(pts, dirs)[1]


@pytest.fixture(scope="module")
def grids(renderer):
    """(lattice index, network) -> the GPU's sigma grid (nz, ny, nx), computed once and left unchanged."""
    out = {}
    for k, (lo, step, dims) in enumerate(LATTICES):
        for name in NETS:
            sig, bits, count, bounds = _net(renderer, name).density_grid(lo, step, dims)
            assert bits is None and count is None and bounds is None and sig.shape == dims[::-1] and sig.dtype == np.float32
            sig.setflags(write=False)
            out[k, name] = sig
    return out


# ---- 1. density_batch = the sigma of forward_batch, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 4096])
def test_density_batch_equals_forward_batch_sigma(renderer, device, name, n):
    g = golden("forward_batch_4096.npz")
    start = 0 if n == 4096 else 100
    pts = np.ascontiguousarray(g["pts"][:, start:start + n]); dirs = np.ascontiguousarray(g["dirs"][start:start + n])
    net = _net(renderer, name)
    _, want = net.forward_batch(pts, dirs)
    got = net.density(pts)
    assert got.shape == (n,) and got.dtype == np.float32
    diff = np.flatnonzero(_bits(got) != _bits(want))
    assert diff.size == 0, (diff[:8], got[diff[:8]], want[diff[:8]])
    # the device entry point, on the default stream
    d_pts, d_sig = device.upload(pts), device.upload(np.full(n, -1.0, np.float32))
    net.density_device(d_pts, d_sig, n)
    assert _same_bits(device.download(d_sig, (n,), np.float32), want)


def test_density_batch_empty(renderer):
    assert renderer.fine.density(np.zeros((3, 0), np.float32)).shape == (0,)


# ---- 2. density_batch against the live oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_density_batch_against_the_oracle(renderer, oracle_nets, name):
    g = golden("forward_batch_4096.npz")
    got = _net(renderer, name).density(g["pts"])
    want = _oracle_sigma(oracle_nets, name, g["pts"])
    err = np.abs(got - want) / (1 + np.abs(want))
    print(f"\n{name}: max |dsigma| / (1 + |sigma|) = {err.max():.3e}")
    assert np.all(np.abs(got - want) <= SIGMA_TOL * (1 + np.abs(want)))
    assert (want > 0).any() and (want == 0).any()


# ---- 3. the lattice grid = density_batch at the host-built points, bit for bit; the oracle gate ------------------------------------------
@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("k", range(len(LATTICES)), ids=LATTICE_IDS)
def test_grid_equals_density_batch_at_host_points(renderer, oracle_nets, grids, k, name):
    lo, step, dims = LATTICES[k]
    pts = lattice_points(lo, step, dims)
    grid = grids[k, name]
    at_points = _net(renderer, name).density(pts)
    diff = np.flatnonzero(_bits(grid.ravel()) != _bits(at_points))
    assert diff.size == 0, (diff[:8], grid.ravel()[diff[:8]], at_points[diff[:8]])
    want = _oracle_sigma(oracle_nets, name, pts)
    err = np.abs(grid.ravel() - want) / (1 + np.abs(want))
    print(f"\n{LATTICE_IDS[k]} {name}: max |dsigma| / (1 + |sigma|) = {err.max():.3e}, {np.mean(grid > 0):.1%} of the cells have sigma > 0")
    assert np.all(np.abs(grid.ravel() - want) <= SIGMA_TOL * (1 + np.abs(want)))
    if grid.size >= 30:                                          # neither an all-zero nor an all-positive output can pass
        assert np.mean(grid > 0) >= 0.05 and np.mean(grid == 0) >= 0.05, (np.mean(grid > 0), np.mean(grid == 0))


# ---- 4. occupancy ------------------------------------------------------------------------------------------------------------------------
def _numpy_occupancy(sig, thr):
    occ = sig > np.float32(thr)
    n = occ.size
    packed = np.packbits(occ.ravel(), bitorder="little")
    words = np.concatenate([packed, np.zeros(-packed.size % 4, np.uint8)]).view("<u4")
    nz, ny, nx = occ.shape
    if occ.any():
        iz, iy, ix = np.nonzero(occ)
        bounds = (ix.min(), iy.min(), iz.min(), ix.max(), iy.max(), iz.max())
    else:
        bounds = (nx, ny, nz, -1, -1, -1)
    return occ, words, int(occ.sum()), tuple(int(v) for v in bounds), n


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("k", range(len(LATTICES)), ids=LATTICE_IDS)
def test_occupancy_words_count_and_bounds(native, renderer, grids, k, name, thr):
    lo, step, dims = LATTICES[k]
    net = _net(renderer, name)
    sig, bits, count, bounds = net.density_grid(lo, step, dims, threshold=thr)
    assert _same_bits(sig, grids[k, name])                        # the sigma store is the same with the occupancy fused in
    occ, words, n_occ, want_bounds, n = _numpy_occupancy(sig, thr)
    assert bits.dtype == np.uint32 and bits.shape == ((n + 31) // 32,)
    assert np.array_equal(bits, words), (bits[:4], words[:4])
    if n % 32:
        assert int(bits[-1]) >> (n % 32) == 0                     # the bits behind the last cell
    assert count == n_occ == sum(bin(int(w)).count("1") for w in bits)
    assert bounds == want_bounds
    if thr == 1e9:
        assert count == 0 and bounds == (dims[0], dims[1], dims[2], -1, -1, -1) and not bits.any()
    assert np.array_equal(native.unpack_occupancy(bits, dims), occ)
    # occupancy alone: sigma is never materialised, the words are the same
    none, bits2, count2, bounds2 = net.density_grid(lo, step, dims, threshold=thr, want_sigma=False)
    assert none is None and np.array_equal(bits2, bits) and count2 == count and bounds2 == bounds


def test_grid_device_entry_point(renderer, device, grids):
    k = 3
    lo, step, dims = LATTICES[k]
    n = dims[0] * dims[1] * dims[2]
    n_words = (n + 31) // 32
    d_sig, d_bits = device.upload(np.full(n, -1.0, np.float32)), device.upload(np.full(n_words, 0xffffffff, np.uint32))
    assert renderer.fine.density_grid_device(lo, step, dims, d_sig, 10.0, d_bits) is None
    sig = device.download(d_sig, dims[::-1], np.float32)
    assert _same_bits(sig, grids[k, "fine"])
    _, words, n_occ, want_bounds, _ = _numpy_occupancy(sig, 10.0)
    assert np.array_equal(device.download(d_bits, (n_words,), np.uint32), words)
    d_bits2 = device.upload(np.full(n_words, 0xffffffff, np.uint32))
    stats = renderer.fine.density_grid_device(lo, step, dims, None, 10.0, d_bits2, want_stats=True)   # synchronises
    assert stats == (n_occ, want_bounds) and np.array_equal(device.download(d_bits2, (n_words,), np.uint32), words)


# ---- 5. other behaviour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_mirrored_and_degenerate_lattices(renderer, name):
    """Every product and sum of this lattice is exact in f32 (dyadic lo and step), so walking it backwards with negative steps visits the
    same points: the mirrored grid, bit for bit.  A zero step repeats one plane."""
    net = _net(renderer, name)
    lo, step, dims = np.float32([-0.5, -0.75, 0.0]), np.float32([0.125, 0.25, 0.5]), (9, 7, 3)
    fwd = net.density_grid(lo, step, dims)[0]
    hi = (lo + step * (np.float32(dims) - 1)).astype(np.float32)
    shape = (3,) + dims[::-1]
    assert np.array_equal(lattice_points(hi, -step, dims).reshape(shape), lattice_points(lo, step, dims).reshape(shape)[:, ::-1, ::-1, ::-1])   # the premise
    back = net.density_grid(hi, -step, dims)[0]
    assert _same_bits(back, fwd[::-1, ::-1, ::-1]) and (fwd > 0).any() and (fwd == 0).any()
    x_only = net.density_grid((hi[0], lo[1], lo[2]), (-step[0], step[1], step[2]), dims)[0]
    assert _same_bits(x_only, fwd[:, :, ::-1])
    flat = net.density_grid(lo, np.float32([0.0, 0.25, 0.5]), dims)[0]
    assert _same_bits(flat, np.repeat(fwd[:, :, :1], 9, axis=2))


def test_determinism_and_network_selection(renderer, grids):
    k = 4
    lo, step, dims = LATTICES[k]
    for name in NETS:
        again = _net(renderer, name).density_grid(lo, step, dims, threshold=10.0)
        assert _same_bits(again[0], grids[k, name])
        assert np.array_equal(again[1], _net(renderer, name).density_grid(lo, step, dims, threshold=10.0, want_sigma=False)[1])
    assert not np.array_equal(grids[k, "coarse"], grids[k, "fine"])
    g = golden("forward_batch_4096.npz")
    assert not np.array_equal(renderer.coarse.density(g["pts"][:, :256]), renderer.fine.density(g["pts"][:, :256]))


def test_unloaded_context_is_a_state_error(native):
    with native.Renderer(0) as r:
        net = native.Network(r, 1)
        with pytest.raises(native.NerfError) as e:
            net.density_grid((0, 0, 0), (0.1, 0.1, 0.1), (2, 2, 2), threshold=0.0)
        assert e.value.code == -6 and "not loaded" in e.value.msg
        with pytest.raises(native.NerfError) as e:
            net.density(np.zeros((3, 5), np.float32))
        assert e.value.code == -6
        with pytest.raises(native.NerfError) as e:                # argument errors come first, with a live context as without one
            net.density_grid((0, 0, 0), (0.1, 0.1, 0.1), (2, 0, 2))
        assert e.value.code == -1


def test_argument_errors_with_a_live_context(native, renderer):
    for kw in (dict(dims=(46341, 46341, 1)), dict(threshold=-1.0), dict(threshold=float("nan")), dict(lo=(0, float("inf"), 0)), dict(want_sigma=False)):
        args = dict(lo=(0, 0, 0), step=(0.1, 0.1, 0.1), dims=(2, 2, 2)); args.update(kw)
        with pytest.raises(native.NerfError) as e:
            renderer.fine.density_grid(**args)
        assert e.value.code == -1, (kw, e.value)


def test_cli_writes_the_library_bytes(renderer, tmp_path):
    k = 3
    lo, step, dims = LATTICES[k]
    exe = os.path.join(ROOT, "nerf-rs_amd", "nerf_cli")
    exact = lambda v: ",".join(repr(float(np.float32(x))) for x in v)     # the f32 values, spelled so that they parse back to themselves
    raw, words = tmp_path / "g.raw", tmp_path / "g.bits"
    res = subprocess.run([exe, "--scene", SCENE, "--density-grid", ",".join(str(d) for d in dims), "--grid-lo", exact(lo), "--grid-step", exact(step),
                          "--grid-net", "coarse", "--grid-threshold", "10", "--grid-out", str(raw), "--grid-occupancy", str(words)],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    sig, bits, count, bounds = renderer.coarse.density_grid(lo, step, dims, threshold=10.0)
    assert raw.read_bytes() == sig.astype("<f4").tobytes() and words.read_bytes() == bits.astype("<u4").tobytes()
    assert f"density grid 33 x 7 x 3 (coarse network): 693 cells, {count} with sigma > 10" in res.stdout
    assert f"x {bounds[0]}..{bounds[3]} y {bounds[1]}..{bounds[4]} z {bounds[2]}..{bounds[5]}" in res.stdout
    assert "Rendering" not in res.stdout and not (tmp_path / "output.ppm").exists()      # only a grid was asked for: no render
    only_bits = subprocess.run([exe, "--scene", SCENE, "--density-grid", ",".join(str(d) for d in dims), "--grid-lo", exact(lo), "--grid-step", exact(step),
                                "--grid-net", "coarse", "--grid-threshold", "10", "--grid-occupancy", str(tmp_path / "h.bits")],
                               capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert only_bits.returncode == 0 and (tmp_path / "h.bits").read_bytes() == words.read_bytes()
    assert subprocess.run([exe, "--scene", SCENE, "--density-grid", "4,4,4"], capture_output=True, cwd=str(tmp_path)).returncode == 2


# ---- 6. unchanged behaviour ---------------------------------------------------------------------------------------------------------------
def test_render_is_unchanged_by_a_grid_call(native, renderer, samples):
    cam = native.camera_from_samples(samples, 256, 256, 32)
    crop = (96, 104, 64, 48)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    lo, step, dims = LATTICES[5]
    renderer.fine.density_grid(lo, step, dims, threshold=0.0)
    renderer.coarse.density(lattice_points(lo, step, dims))
    after = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    assert before.shape == (48, 64, 3) and _same_bits(after, before)
