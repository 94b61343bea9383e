#!/usr/bin/env python3
"""Quick A/B: render the 800x800 frame a few times with the library named by NERF_MI355X_LIB and print the
device times (ms) of the coarse / fine MLP kernels plus a parity check against the committed C3 crop."""
import os, sys
os.environ.setdefault("NERF_ALLOW_VARIANT", "1")  # these tools exist to time variant builds
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N
n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
size = int(sys.argv[2]) if len(sys.argv) > 2 else 800
dtype = sys.argv[3] if len(sys.argv) > 3 else "f32"
with N.Renderer(0) as r:
    r.load_scene(os.path.join(ROOT, "lego_rust"))
    cam = N.camera_from_samples(os.path.join(ROOT, "lego_rust", "tf_reference_samples.json"), size, size, 64)
    best = None
    for k in range(n):
        img, st = N.render_image(r.coarse, r.fine, cam, 128, seed=0, dtype=dtype, return_stats=True)
        if best is None or st.ms_total < best.ms_total:
            best = st
    msg = ""
    if size == 800:
        g = np.load(os.path.join(ROOT, "tests/golden/crop_c3_800_64_128.npz"))
        x0, y0, w, h = (int(v) for v in g["crop"])
        d = np.abs(img[y0:y0 + h, x0:x0 + w] - g["image"])
        msg = f" crop max|d| {d.max():.2e} mean {d.mean():.2e}"
    import ctypes as C
    mhz = C.c_double(0)
    if os.environ.get("NERF_DEBUG_CLOCK") and r._L.nerf_debug_shader_clock_mhz(r.handle, C.byref(mhz)) == 0:
        msg += f" clock {mhz.value:.0f} MHz"
    peak = 2500.0 if dtype in ("bf16", "bf16x3", "f16x2") else 157.3
    ex = 6.0 if dtype == "bf16x3" else 3.0 if dtype == "f16x2" else 1.0  # executed 16-bit MFMA flops per algorithmic f32 flop
    fl = ex * best.n_fine_points * N.FLOP_PER_POINT_FULL / (best.ms_fine_mlp * 1e-3) / 1e12
    cl = ex * best.n_coarse_points * N.FLOP_PER_POINT_SIGMA / (best.ms_coarse_mlp * 1e-3) / 1e12
    print(f"{os.path.basename(N.lib_path()):34s} total {best.ms_total:8.2f} ms  coarse {best.ms_coarse_mlp:7.2f} ({cl:6.2f} TF)  "
          f"fine {best.ms_fine_mlp:8.2f} ({fl:6.2f} TF = {100 * fl / peak:5.2f}%)  other {best.ms_other:5.2f}  "
          f"rays/s {best.n_rays / best.ms_total * 1e3:9.0f}{msg}", flush=True)
