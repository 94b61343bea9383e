"""A context gives back every device buffer it grew (nerf_destroy; -m gpu).

In one process, three times over: create a Renderer, load the lego networks, make one small call of every family that grows a buffer of
the context, destroy the renderer, read the device's free memory.  The families: an 8 x 8 image plain, with ssaa=2 + aux, as rgba8, with
skip_dead in bf16x3 and with certify_zero; a 64-ray batch with per-ray origins and bounds, the same with normals, clipped, and clipped +
certified; density_grid, extract_mesh(keep_largest=1) and density_gradient on a 16^3 lattice; forward_batch of 256 points; stage_ray_dirs.

Free memory after cycle 3 must equal free memory after cycle 2 (cycle 1 also pays for what the process keeps for good: code objects, the
runtime's own pools).  Allowance: RESIDUE bytes, what the commit before the context's buffers became self-enumerating showed for this
very test on an MI355X -- measured 0.  Every output of cycles 2 and 3 equals cycle 1's bit for bit."""
import os
import subprocess
import sys

import pytest

from conftest import SCENE

pytestmark = pytest.mark.gpu

RESIDUE = 0


def test_destroy_gives_back_every_buffer_and_cycles_repeat_bit_for_bit():
    """tests/helpers/context_lifetime_child.py runs the three cycles and compares their outputs.  A process of its own, because the free
    memory is read through torch, which must load its HIP runtime before the library's (see tests/helpers/ray_batch_torch_child.py)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "context_lifetime_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    words = p.stdout.strip().splitlines()[-1].split()
    assert words[0] == "free" and len(words) == 4, p.stdout[-2000:]
    free = [int(w) for w in words[1:]]
    print(f"free device memory after cycles 1..3: {free}, residue {free[1] - free[2]} B")
    assert abs(free[1] - free[2]) <= RESIDUE, free
