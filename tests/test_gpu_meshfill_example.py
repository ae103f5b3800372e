"""examples/fill_and_measure_mesh.py run as written at a 24^3 grid, in a child process: it prints measure() before (closed=False)
and after fill_holes (closed=True, a positive volume near the spherical cap's) and writes an OBJ that load_obj reads back closed."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_fill_example(tmp_path):
    from swnerf import mesh
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fill_and_measure_mesh.py"), str(tmp_path), "24"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    lines = r.stdout.splitlines()
    first = next(l for l in lines if l.startswith("as extracted"))
    second = next(l for l in lines if l.startswith("holes filled"))
    assert "closed=False" in first and "closed=True" in second and lines.index(first) < lines.index(second)
    vol = float(re.search(r"volume (-?[0-9.]+)", second).group(1))
    pct = float(re.search(r": ([0-9.]+) % after", r.stdout).group(1))
    assert vol > 0 and abs(pct - 100) < 3.                           # the margin of the cut-sphere test at the same grid
    m = mesh.measure(mesh.load_obj(str(tmp_path / "mesh_filled.obj")))
    assert m.closed and m.euler == 2 and abs(m.volume - vol) < 1e-4
