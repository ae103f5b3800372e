"""examples/clean_and_measure_mesh.py run as written, in a child process: it writes two OBJs that load_obj reads back; the cleaned
one measures as one closed component whose extents are the object's, the raw one as the whole box of floaters."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_clean_and_measure_example(tmp_path):
    from swnerf import mesh
    R, scale = 48, 0.25
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "clean_and_measure_mesh.py"), str(tmp_path), str(R), str(scale), "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "raw    :" in r.stdout and "cleaned:" in r.stdout and "closed = True" in r.stdout
    raw = mesh.load_obj(str(tmp_path / "mesh_raw_scaled.obj"))
    cleaned = mesh.load_obj(str(tmp_path / "mesh_clean_scaled.obj"))
    assert len(raw[1]) > len(cleaned[1]) > 0 and cleaned[3] is not None
    before, after = mesh.measure(raw), mesh.measure(cleaned)
    assert before.n_components > 10 and before.extents.max() > 1.5 * scale
    assert after.n_components == 1 and after.closed and after.boundary_edges == 0 and after.euler == 2
    h = 2. / (R - 1)
    want = 2 * scale * np.array([0.6, 0.45, 0.3])
    assert np.abs(after.extents - want).max() <= 2 * h * scale              # a grid cell either side
    vol = 4. / 3. * np.pi * scale ** 3 * 0.6 * 0.45 * 0.3
    assert abs(after.volume - vol) <= 0.05 * vol and after.area > 0
